// qtos_planner.hip -- C ABI (include/qtos_planner.h) over the gfx950 kernels: the handle, the solver's entries (create,
// submit / poll, report, debug, self-test) over kernels.hpp and kkt*.hpp here, the steps that build the handle in
// planner_create.hpp, the sampler's and the receding loop's entries over window_kernels.hpp in window_api.hpp.  One translation unit.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared qtos_planner.hip -o libqtos_planner.so
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string>
#include <tuple>
#include <map>
#include <memory>
#include <vector>

#include "kernels.hpp"   // (with call_schedule.hpp: the launch schedule of a plan call)
#include "window_kernels.hpp"
#include "kkt2.hpp"
#include "kkt3.hpp"
#include "kkt5.hpp"
#include "csv_writer.hpp"

using namespace qtos;

#define HIPCHK(p, call)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (p)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
      return e_ == hipErrorOutOfMemory ? -3 : -2;                                             \
    }                                                                                         \
  } while (0)

enum class Kkt { kkt2, kkt3, kkt5 };                      // the factor + solve kernel (choose_kernel)
// One host analysis.  Symbolic::build writes into its model (goff, g_doubles, dyn_chunk): a model per variant; moving is safe.
struct Analysis { HostModel M; Symbolic S; };

struct QtosPlanner : Analysis {   // (the analysis the planner runs: choose_kernel)
  DevPlan dp;
  SamplePlan sp;
  SamplePlan *d_sp = nullptr;  // sp in device memory (k_handover reads the tables through a pointer)
  const int *d_stance[NEE] = {nullptr, nullptr, nullptr, nullptr};   // per foot and polynomial of its motion spline: 1 stance, 0 swing (k_plan_check)
  int device = 0, max_batch = 0;
  std::vector<void *> allocs;  // everything to free
  // workspace
  DevWork wk;
  double *d_start = nullptr, *d_goal = nullptr, *d_nodes = nullptr, *d_warm = nullptr;
  int *d_map = nullptr;
  double *d_height = nullptr;
  size_t height_cnt = 0;                                   // doubles of d_height (qtos_set_heightfields_device keeps a buffer of the same size)
  hipEvent_t ev_height = nullptr;                          // behind the copy of qtos_set_heightfields_device: whoever reads the terrain on another stream waits for it
  hipStream_t height_stream = nullptr;
  bool height_pending = false;
  hipStream_t own_stream = nullptr;   // stream of the host-pointer entry points (non-blocking: other handles / streams are not synchronised)
  long long *d_totals = nullptr;      // converged problems, iterations: tallied at the end of every plan call (qtos_plan_totals)
  hipStream_t last_stream = nullptr;
  double *d_table = nullptr, *d_tab_dx = nullptr, *d_tab_dy = nullptr;   // nominal-plan table (qtos_set_init_table)
  // A call is served by one or more LANES.  A lane owns everything one host-driven Newton loop needs: the stream its kernels
  // run on (lane 0: the caller's; the others: streams of the planner), a side stream for the chord solve that runs next to a
  // factorisation, the pinned count slots its iterations report to, its events and its two device counters.  A call of more
  // problems than the GPU has compute units is cut into contiguous parts, one per lane: the late iterations of a part's
  // stragglers then run side by side with the other parts' full grids instead of holding the whole call -- the reference's
  // queue of probes (QTOS/generateHeightField.py:375-377) inside ONE call.  The parts never meet: the plans are bit for bit
  // those of a single lane (QTOS_LANES=1).
  struct Lane : LaneProgress {               // (call_schedule.hpp: how far the lane is, and what its last call's slots ran)
    int B = 0, b0 = 0;                       // problems, first problem
    unsigned spins = 0;                      // polls that found no counts yet
    hipStream_t st = nullptr;                // where this lane's kernels go in the call in flight
    hipStream_t own = nullptr, side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_done = nullptr;
    DevWork W;
    int *h_active = nullptr;      // pinned + mapped: the count slots of call_schedule.hpp (SlotLayout::counts_at)
    int *h_active_dev = nullptr;  // the same memory as the device sees it (k_post_counts stores there: no copy engine between two kernels)
    int *d_n_active = nullptr;    // the lane's four device counters (DevWork::n_active)
    std::vector<hipEvent_t> ev;   // SlotLayout::ev, EV_CALL_BEGIN, EV_CALL_END
  };
  std::vector<Lane> lanes;
  int lanes_used = 1, lane_chunk = 256;      // lanes of the call in flight; problems per lane above which a call is cut (the GPU's compute units)
  bool call_open = false;
  // per-solve report (qtos_set_report): the flag, and what the last call latched of it (qtos_plan_report)
  bool report = false, last_report = false;
  int last_B = 0;
  unsigned seq = 0;                          // sequence number of the call in flight, stamped into the count words (k_post_counts)
  hipStream_t call_stream = nullptr;
  hipEvent_t ev_in = nullptr;                // the caller's stream at submit time: the other lanes start behind it
  Kkt kkt = Kkt::kkt2;               // the factor + solve kernel (choose_kernel)
  QtosEnv env;                       // the environment as qtos_planner_create found it (env.hpp; qtos_env reports it)
  int last_iters = 1;                // iterations the last call took: the blind iterations of the next (blind_slots)
  int spec_cap = 1;                  // limit of the blind iterations (qtos_set_speculation): 1 = off
  // Launch pattern (round 6): the solve kernels every launch slot of the handle's last two calls needed, as far as the two
  // agree -- the walk's and the trot's batches take kkt, kkt, kkt, chord every time.  qtos_plan_submit queues that prefix at
  // once, without a look at the counts; the counts behind its last slot say whether anything is left (qtos_plan_poll goes on
  // informed) and whether a problem found the wrong kernel (it sat the launch out, kernels.hpp k_step: the pattern is cut in
  // front of that slot).
  LaunchPattern pattern;
  bool per_kernel_events = true;     // HIP events around every solve kernel and behind every slot (qtos_last_timing*); qtos_set_kernel_events(0): only the call's first and last
  SlotLayout slots;                  // where a lane's count slots and events sit (max_slots: create_lanes)
  std::atomic<int> busy{0};
  size_t kkt_lds = 0, eval_lds = 0;
  void (*chord_fn)(DevPlan, DevWork, int) = nullptr; // k_chord instantiated for this front size (null: chord steps off)
  void (*kkt_fn)(DevPlan, DevWork, int) = nullptr;   // k_kkt / k_kkt2 instantiated for this front size
  int kkt_threads = KT;
  std::string err;
  bool on_device = false;   // hipSetDevice(device) has succeeded (create_planner): from here on the handle may own device objects

  // The handle owns what it allocates.  One that has made no HIP call yet makes none when it goes.
  ~QtosPlanner() {
    if (!on_device) return;
    (void)hipSetDevice(device);
    for (void *a : allocs) (void)hipFree(a);
    for (auto &L : lanes) {
      for (hipEvent_t e : L.ev)
        if (e) (void)hipEventDestroy(e);
      if (L.h_active) (void)hipHostFree(L.h_active);
      for (hipStream_t s : {L.own, L.side})
        if (s) (void)hipStreamDestroy(s);
      for (hipEvent_t e : {L.ev_fork, L.ev_join, L.ev_done})
        if (e) (void)hipEventDestroy(e);
    }
    for (void *q : {(void *)d_table, (void *)d_tab_dx, (void *)d_tab_dy, (void *)d_height, (void *)d_totals})
      if (q) (void)hipFree(q);
    for (hipEvent_t e : {ev_in, ev_height})
      if (e) (void)hipEventDestroy(e);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }

  template <class T>
  int upload(const std::vector<T> &v, const T **out) {
    T *d = nullptr;
    size_t bytes = std::max<size_t>(1, v.size()) * sizeof(T);
    HIPCHK(this, hipMalloc((void **)&d, bytes));
    allocs.push_back(d);
    if (!v.empty()) HIPCHK(this, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = d;
    return 0;
  }
  template <class T>
  int alloc(T **out, size_t count) {
    T *d = nullptr;
    HIPCHK(this, hipMalloc((void **)&d, std::max<size_t>(1, count) * sizeof(T)));
    HIPCHK(this, hipMemset(d, 0, std::max<size_t>(1, count) * sizeof(T)));
    allocs.push_back(d);
    *out = d;
    return 0;
  }
};

// The device copies of one host call's arrays (the host forms of window_api.hpp): buffers of the call's own, so the handle's
// staging buffers are not touched and a host form may run while a call is open.  Counts are in elements.  An array that was
// not given (a null pointer) gets no copy and stays a null pointer.  pad: elements allocated behind those that are copied, so
// that an empty array is a pointer still.  The copies are blocking ones on the null stream, around a launch on the null stream.
// The first HIP call that fails sets rc (and the handle's err, as HIPCHK does) and the later ones are left out: the form looks
// at rc once, before it launches.  Everything is freed when the call returns, whichever way.
namespace {   // (no symbols of it leave the library)
class Staging {
 public:
  int rc = 0;
  explicit Staging(QtosPlanner *p) : p(p) {}
  Staging(const Staging &) = delete;
  Staging &operator=(const Staging &) = delete;
  ~Staging() { for (const Buf &b : bufs) (void)hipFree(b.d); }
  template <class T> T *in(const T *h, size_t count, size_t pad = 0) { return (T *)add(h, nullptr, count * sizeof(T), pad * sizeof(T)); }
  template <class T> T *out(T *h, size_t count, size_t pad = 0) { return (T *)add(nullptr, h, count * sizeof(T), pad * sizeof(T)); }
  // copied in as well, so what the kernel does not write comes back as it was; back = false: not copied back after all
  template <class T> T *inout(T *h, size_t count, size_t pad = 0, bool back = true) {
    return (T *)add(h, back ? h : nullptr, count * sizeof(T), pad * sizeof(T));
  }
  // behind the kernel: every out and inout array back to the host
  int download() {
    for (const Buf &b : bufs)
      if (b.back && b.bytes) HIPCHK(p, hipMemcpy(b.back, b.d, b.bytes, hipMemcpyDeviceToHost));
    return 0;
  }

 private:
  struct Buf { void *d; void *back; size_t bytes; };
  QtosPlanner *p;
  std::vector<Buf> bufs;
  void *add(const void *from, void *back, size_t bytes, size_t pad) {
    if (rc || (!from && !back)) return nullptr;
    bufs.push_back({nullptr, back, bytes});
    rc = upload(bufs.back().d, from, bytes, pad);
    return bufs.back().d;
  }
  int upload(void *&d, const void *from, size_t bytes, size_t pad) {
    HIPCHK(p, hipMalloc(&d, bytes + pad));
    if (from && bytes) HIPCHK(p, hipMemcpy(d, from, bytes, hipMemcpyHostToDevice));
    return 0;
  }
};
}  // namespace

// k_kkt is compiled once per front size (multiples of 16 up to 128): the LDS layout and every tile
// loop bound are compile-time constants
// k_kkt2 (16 waves per problem): fronts up to 208 slots
static void (*kkt2_kernel(int F, bool cont))(DevPlan, DevWork, int) {
#define QTOS_KKT2(f) case f: return cont ? k_kkt2<f, true> : k_kkt2<f, false>;
  switch (F) {
#ifdef QTOS_DEV_F128   // (development builds: the benchmark's fronts only, a quarter of the compile time)
    QTOS_KKT2(112) QTOS_KKT2(128)
#else
    QTOS_KKT2(16) QTOS_KKT2(32) QTOS_KKT2(48) QTOS_KKT2(64) QTOS_KKT2(80) QTOS_KKT2(96) QTOS_KKT2(112) QTOS_KKT2(128)
#endif
#if !defined(QTOS_DEV_SMALL) && !defined(QTOS_DEV_F128)
    QTOS_KKT2(144) QTOS_KKT2(160) QTOS_KKT2(176) QTOS_KKT2(192) QTOS_KKT2(208)
#endif
  }
#undef QTOS_KKT2
  return nullptr;
}
// k_kkt3 (k_kkt2's records and arithmetic, the assembly on the waves that idle in phase AB): fronts up to 128 slots
static void (*kkt3_kernel(int F))(DevPlan, DevWork, int) {
#define QTOS_KKT3(f) case f: return k_kkt3<f, 1>;
#ifndef QTOS_DEV_F128
  switch (F) { QTOS_KKT3(16) QTOS_KKT3(32) QTOS_KKT3(48) QTOS_KKT3(64) QTOS_KKT3(80) QTOS_KKT3(96) QTOS_KKT3(112) QTOS_KKT3(128) }
#endif
#undef QTOS_KKT3
  return nullptr;
}
// k_kkt5 (two 16-pivot stages per set of barriers, twelve waves): fronts up to 144 slots
static void (*kkt5_kernel(int F))(DevPlan, DevWork, int) {
#define QTOS_KKT5(f) case f: return k_kkt5<f>;
#ifdef QTOS_DEV_F128
  switch (F) { QTOS_KKT5(112) QTOS_KKT5(128) }
#else
  switch (F) { QTOS_KKT5(96) QTOS_KKT5(112) QTOS_KKT5(128) QTOS_KKT5(144) }
#endif
#undef QTOS_KKT5
  return nullptr;
}
static void (*chord_kernel(int F))(DevPlan, DevWork, int) {
#define QTOS_CHORD(f) case f: return k_chord<f>;
  switch (F) {
#ifdef QTOS_DEV_F128
    QTOS_CHORD(112) QTOS_CHORD(128)
#else
    QTOS_CHORD(16) QTOS_CHORD(32) QTOS_CHORD(48) QTOS_CHORD(64) QTOS_CHORD(80) QTOS_CHORD(96) QTOS_CHORD(112) QTOS_CHORD(128)
#endif
#if !defined(QTOS_DEV_SMALL) && !defined(QTOS_DEV_F128)
    QTOS_CHORD(144) QTOS_CHORD(160) QTOS_CHORD(176) QTOS_CHORD(192) QTOS_CHORD(208)
#endif
  }
#undef QTOS_CHORD
  return nullptr;
}

// The analysis of an order rule and variant (pair mode, record cap; the default has neither): 0, -1 / 1 failed
static int build_analysis(Analysis &A, const QtosParams &params, const QtosEnv &env, int order_rule, bool pair = false, int cap = 0) {
  A = Analysis();
  A.M.order_rule = order_rule;
  A.S.env = env; A.S.cell_mode = 2; A.S.pair_mode = pair; A.S.rec_cap_ints = cap;
  if (A.M.build(params)) return -1;
  return A.S.build(A.M) ? 1 : 0;
}
static int print_error(const Analysis &A, int rc) { fprintf(stderr, "qtos: %s\n", (rc < 0 ? A.M.err : A.S.err).c_str()); return -1; }

// Which time keys the elimination order uses (model.hpp HostModel::order_rule): the rules in the order of preference, each
// analysed once.  On a reduced base the rules of the mask are analysed (none given: 2 and 1, the automatic choice): the smaller
// front comes first, then the fewer stages, then the order that needs no continuation records, then 2 before 1 before 0; a rule
// whose analysis fails comes last with front 0.  Rule 0 -- the order of rounds 1 - 5 -- has the smallest front on some short
// horizons and is NOT in the automatic choice there: its KKT solve loses up to six digits on short trots (model.hpp).
// QTOS_ORDER=0 | 1 | 2 forces one rule, whatever the mask.  The candidates do not talk.
struct Candidate {
  int rule, front, stages, cont;
  bool ok;
  std::unique_ptr<Analysis> A;   // the default variant of the rule, unless it failed or the analysis is to talk (QTOS_DEBUG_SYMBOLIC*, QTOS_DUMP_FIRST)
};
static std::vector<Candidate> order_candidates(const QtosParams &params, const QtosEnv &env, int rules_mask) {
  QtosEnv quiet = env;
  quiet.debug = 0; quiet.dump_first.clear();
  const bool keep = !env.debug && env.dump_first.empty();
  bool reduced = true;
  auto analyse = [&](int rule) {
    Candidate c = {rule, 0, 0, 0, false, std::make_unique<Analysis>()};
    c.ok = build_analysis(*c.A, params, quiet, rule) == 0;
    if (c.ok) { c.front = c.A->S.front; c.stages = c.A->S.n_stages; c.cont = c.A->S.n_continuation() > 0; }
    reduced = c.A->M.reduce_base != 0;
    if (!c.ok || !keep) c.A.reset();
    return c;
  };
  std::vector<Candidate> out;
  if (env.order >= 0) { out.push_back(analyse(env.order)); return out; }
  // (rules 1 and 2 move the B-spline coefficients of the reduced base: without it -- every base row in the system, the
  //  configuration the internals' tests pin -- the order of rounds 1 - 5 stays)
  if (!params.reduce_base) { out.push_back(analyse(0)); return out; }
  const int mask = (rules_mask & 7) ? (rules_mask & 7) : 6;
  for (int rule : {2, 1, 0}) {
    if (!((mask >> rule) & 1)) continue;
    Candidate c = analyse(rule);
    // (the model kept the full base, a short horizon or unequal polynomial durations: rule 0 alone)
    if (c.ok && !reduced) { out.clear(); out.push_back(analyse(0)); return out; }
    out.push_back(std::move(c));
  }
  std::stable_sort(out.begin(), out.end(), [](const Candidate &a, const Candidate &b) {   // (stable: 2 before 1 before 0 among equals)
    return std::make_tuple(!a.ok, a.front, a.stages, a.cont) < std::make_tuple(!b.ok, b.front, b.stages, b.cont);
  });
  return out;
}
// The rule a planner runs and qtos_analyze* describes: the first candidate of the automatic mask.  `won` takes its analysis
// where the candidate kept it (`built`); the caller builds the others, which then talk or say why they fail.
static int pick_order_rule(const QtosParams &params, const QtosEnv &env, Analysis &won, bool &built) {
  std::vector<Candidate> c = order_candidates(params, env, 0);
  if (env.debug && c.size() > 1) fprintf(stderr, "qtos: elimination order rule %d (front %d, %d stages)\n", c[0].rule, c[0].front, c[0].stages);
  built = c[0].A != nullptr;
  if (built) won = std::move(*c[0].A);
  return c[0].rule;
}

// What the qtos_analyze* entry points describe: the default variant, whatever a planner would run
static int analyze_host(const QtosParams &params, const QtosEnv &env, Analysis &A) {
  bool built;
  const int rule = pick_order_rule(params, env, A, built);
  const int rc = built ? 0 : build_analysis(A, params, env, rule);
  return rc ? print_error(A, rc) : 0;
}
static size_t kkt_lds_bytes(Kkt k, const Symbolic &S) {
  switch (k) {
    case Kkt::kkt5: return Kkt5Lds::of(S.front).bytes(S.n_stages, S.max_srec, S.max_drec, S.n_cells);
    default: return Kkt2Lds::of(S.front).bytes(S.n_stages, S.max_srec, S.max_drec, S.n_cells);   // (k_kkt2 and k_kkt3: one layout)
  }
}
// the kernel's name as rocprofv3 lists it (qtos_kkt_kernel, qtos_analyze_kernel)
static int kkt_kernel_name(Kkt k, const Symbolic &S, char *buf, int n) {
  const size_t room = buf && n > 0 ? (size_t)n : 0;
  switch (k) {
    case Kkt::kkt5: return snprintf(buf, room, "k_kkt5<%d>", S.front);
    case Kkt::kkt3: return snprintf(buf, room, "k_kkt3<%d, 1>", S.front);
    default: return snprintf(buf, room, "k_kkt2<%d%s>", S.front, S.n_continuation() > 0 ? ", true" : "");
  }
}

// Which factor + solve kernel, and the analysis it runs on; 0, or -1 where the analysis fails.  k_kkt3<F, 1> is the default up
// to 112 slots (128 once QTOS_KKT is set): k_kkt2's records and arithmetic -- bit-identical plans -- with the assembly on the
// waves idle in phase AB (-5 % per launch on 112 slots, -6 % on 96, +4 % on 128: profiles/r04_experiments).  k_kkt2 takes the
// rest, with smaller records (heavy stages spill into continuation records) while they do not fit the LDS next to the panels.
// QTOS_KKT=6: k_kkt5 on the pair-mode analysis where it applies; 2 forces k_kkt2; 3 and 5 (rounds 4 - 5) left the library.
// order_rule >= 0: that rule instead of the pick (qtos_planner_create_checked builds its candidates so; the same path as QTOS_ORDER).
// `pre`: the default variant of that rule where the caller has built it (taken, as the pick's winner is).
static int choose_kernel(const QtosParams &params, const QtosEnv &env, Kkt &kind, Analysis &A, int order_rule = -1, Analysis *pre = nullptr) {
  Analysis def; bool have_def = false;   // the default variant: the order pick's winner, or built below
  const int rule = order_rule >= 0 ? order_rule : pick_order_rule(params, env, def, have_def);
  if (order_rule >= 0 && pre) { def = std::move(*pre); have_def = true; }
  int forced = env.kkt;
  if (forced == 3 || forced == 5) { fprintf(stderr, "qtos: QTOS_KKT=%d selected an experiment of rounds 4 - 5 that left the library (scratch/experiments/): default kernel\n", forced); forced = 0; }
  if (forced == 6) {   // (k_kkt5: a front of 96 .. 144 slots, no continuation records, within the LDS)
    const int rc = build_analysis(A, params, env, rule, true);
    if (rc < 0) return print_error(A, rc);
    const Symbolic &S = A.S;
    const bool ok = rc == 0 && kkt5_kernel(S.front) != nullptr && !(S.pack_src.size() & 1) && S.n_continuation() == 0 && kkt_lds_bytes(Kkt::kkt5, S) <= LDS_LIMIT;
    if (env.debug) fprintf(stderr, "qtos: k_kkt5 %s (front %d, %s)\n", ok ? "selected" : "not applicable", S.front, S.err.c_str());
    if (ok) { kind = Kkt::kkt5; return 0; }
  }
  const int def_rc = have_def ? 0 : build_analysis(def, params, env, rule);
  if (def_rc < 0) return print_error(def, def_rc);
  if (forced != 2) {
    const Symbolic &S = def.S;
    const bool ok = def_rc == 0 && S.front <= (forced ? 128 : 112) && !(S.pack_src.size() & 1) && S.n_continuation() == 0 && kkt_lds_bytes(Kkt::kkt3, S) <= LDS_LIMIT;
    if (env.debug) fprintf(stderr, "qtos: k_kkt3 %s (%s)\n", ok ? "selected" : "not applicable", S.err.c_str());
    if (ok) { kind = Kkt::kkt3; A = std::move(def); return 0; }
  }
  kind = Kkt::kkt2;
  for (int cap : {0, 4096, 3072, 2048}) {
    int rc;
    if (cap == 0) { rc = def_rc; A = std::move(def); }
    else rc = build_analysis(A, params, env, rule, false, cap);
    if (rc) return print_error(A, rc);
    if (kkt_lds_bytes(Kkt::kkt2, A.S) <= LDS_LIMIT) break;
  }
  return 0;
}

extern "C" {
__global__ void k_debug_eval(DevPlan P, DevWork W, int B);

const char *qtos_last_error(const QtosPlanner *p) { return p ? p->err.c_str() : "null planner"; }

void qtos_planner_destroy(QtosPlanner *p) { if (p) delete p; }

#include "planner_create.hpp"

int qtos_planner_create(const QtosParams *params, int max_batch, int device, QtosPlanner **out) {
  return create_planner(params, max_batch, device, QtosEnv::parse(), -1, out);   // (a planner reads the environment here, or in qtos_planner_create_checked)
}

static void fill_dims(const HostModel &M, const Symbolic &S, QtosDims *d) {
  std::memset(d, 0, sizeof(*d));
  d->n_vars = M.n_vars; d->n_cons = M.n_cons;
  d->n_free = 0;
  for (int v = 0; v < M.n_vars; ++v) d->n_free += M.is_free(v) ? 1 : 0;   // (the NLP's count; with reduce_base the KKT system has fewer: n_unknowns)
  for (int r = 0; r < M.n_cons; ++r) {
    const bool eq = M.con_lo[r] == M.con_hi[r];
    if (eq) d->n_eq++;
    else {
      d->n_ineq++;
      const bool hl = M.con_lo[r] > -1e19, hu = M.con_hi[r] < 1e19;
      if (hl && hu) d->n_ineq_both++;
      else if (hl) d->n_ineq_lower++;
      else d->n_ineq_upper++;
    }
  }
  d->n_eq_work = S.n_eq; d->n_unknowns = S.n_real_unknowns; d->n_stages = S.n_stages;   // (the unknowns of the KKT system; positions incl. the dummy pivots of short stages: n_stages x 16)
  d->pivots = PIV; d->front = S.front;
  d->n_base_nodes = M.n_base_nodes; d->n_dyn_times = (int)M.t_dyn.size(); d->n_rom_times = (int)M.t_rom.size();
  d->n_rows_csv = (int)std::llround(M.T * 1000.0) + 1;
  d->panel_doubles = (long long)S.n_stages * (S.front + 1) * PIV; d->g_doubles = S.g_doubles;
  d->kkt_algorithmic_bytes = S.algorithmic_bytes; d->kkt_flops = S.flops;
  d->envelope = S.envelope; d->max_active = S.max_active; d->order_rule = M.order_rule;
  d->duration = M.T;
}

int qtos_planner_dims(const QtosPlanner *p, QtosDims *d) {
  if (!p || !d) return -1;
  fill_dims(p->M, p->S, d);
  return 0;
}

int qtos_analyze(const QtosParams *params, QtosDims *d, int *stage_active, int max_stages) {
  if (!params || !d) return -1;
  const QtosEnv env = QtosEnv::parse();
  Analysis A;
  if (analyze_host(*params, env, A)) return -1;
  const auto &[M, S] = A;
  fill_dims(M, S, d);
  if (env.debug) { std::vector<SwTask> t; std::vector<int> c, c2; (void)build_sweep_tasks(M, S, t, c, c2); }
  if (stage_active)
    for (int k = 0; k < S.n_stages && k < max_stages; ++k) stage_active[k] = S.stages[k].n_active;
  return 0;
}

// Host-only: the elimination order by position (qtos_debug_structure's `order` without a planner handle): var index, n_vars + row
// for a multiplier, -1 for a dummy pivot; returns the number of positions (n_stages * pivots) or < 0.
int qtos_analyze_order(const QtosParams *params, int *order, int max_positions) {
  if (!params || !order) return -1;
  Analysis A;
  if (analyze_host(*params, QtosEnv::parse(), A)) return -1;
  const Symbolic &S = A.S;
  const int np = S.n_stages * PIV;
  for (int i = 0; i < np && i < max_positions; ++i) order[i] = i < (int)S.order.size() ? S.order[i] : -1;   // (as qtos_debug_structure)
  return np;
}

// Host-only: what a TWO-ENDED elimination of this model's KKT matrix would look like (Symbolic::analyze_two_ended: a chain from
// t = 0 forward, a chain from t = T backward, the unknowns alive across the split time last), and the LDS a workgroup that runs
// both chains would need with the layouts of today's kernel.  out (>= 20 ints):
//   [0] stages today  [1] front today  [2] split stage  [3] stages of chain L  [4] of chain R  [5] separator unknowns
//   [6] separator stages  [7] front of L  [8] of R  [9] of the separator  [10] serial steps  [11] populated peak of L  [12] of R
//   LDS bytes: [13] today's kernel for this model, of which [14] panels, [15] record buffers, [16] cells;
//   [17] two chains with today's layouts (panels, cells and both record buffers twice, the fixed part twice)
//   [18] two chains, LEAN: per chain two panels + the blanked copy, one record buffer holding the dynamic record only (gather
//        tables read from L2), the cells; the fixed part twice   [19] the limit (160 KB - 256 B)
int qtos_analyze_two_ended(const QtosParams *params, int *out, int n_out) {
  if (!params || !out || n_out < 20) return -1;
  Analysis A;
  if (analyze_host(*params, QtosEnv::parse(), A)) return -1;
  const auto &[M, S] = A;
  const Symbolic::TwoEnded t = S.analyze_two_ended(M);
  const int F = S.front, Fc = std::max(t.front_left, t.front_right);
  const Kkt2Lds L = Kkt2Lds::of(F), Lc = Kkt2Lds::of(Fc);
  const size_t rec_b = L.records_bytes(S.max_srec, S.max_drec), cells_b = L.cells_bytes(S.n_cells);
  const size_t total = L.bytes(S.n_stages, S.max_srec, S.max_drec, S.n_cells), fixed_b = L.fixed_bytes(S.n_stages, S.max_srec, S.max_drec, S.n_cells);
  out[0] = S.n_stages; out[1] = F; out[2] = t.split_stage; out[3] = t.stages_left; out[4] = t.stages_right; out[5] = t.sep_unknowns;
  out[6] = t.stages_sep; out[7] = t.front_left; out[8] = t.front_right; out[9] = t.front_sep; out[10] = t.serial_steps;
  out[11] = t.peak_left; out[12] = t.peak_right;
  out[13] = (int)total; out[14] = (int)L.panels_bytes(); out[15] = (int)rec_b; out[16] = (int)cells_b;
  out[17] = (int)(2 * (Lc.panels_bytes(3) + rec_b + cells_b + fixed_b));
  out[18] = (int)(2 * (Lc.panels_bytes(2) + L.dbuf_doubles(S.max_drec) * sizeof(double) + cells_b + fixed_b));
  out[19] = (int)LDS_LIMIT;
  return 0;
}

// Host-only: the schedule the helper waves of the backward sweep follow (build_sweep_tasks).  Per place of a round (16 per
// round, round i runs in step i of the chain, i.e. while it solves stage n_stages - 1 - i): the constraint row (-1: empty),
// the row's entries, and the smallest and largest position (elimination order) of the row's columns.
int qtos_analyze_sweep(const QtosParams *params, int *n_rounds, int *rows, int *entries, int *pos_min, int *pos_max, int max_places) {
  if (!params || !n_rounds) return -1;
  Analysis A;
  if (analyze_host(*params, QtosEnv::parse(), A)) return -1;
  const auto &[M, S] = A;
  std::vector<SwTask> tasks;
  std::vector<int> cpos, c16;
  *n_rounds = build_sweep_tasks(M, S, tasks, cpos, c16);
  if (*n_rounds <= 0) return -4;
  for (int i = 0; i < *n_rounds * SW_ROUND && i < max_places; ++i) {
    const SwTask &t = tasks[i];
    int lo = INT_MAX, hi = -1;
    for (int a = 0; a < t.n && t.row >= 0; ++a) { lo = std::min(lo, cpos[t.cpos_off + a]); hi = std::max(hi, cpos[t.cpos_off + a]); }
    if (rows) rows[i] = t.row;
    if (entries) entries[i] = t.row >= 0 ? t.n : 0;
    if (pos_min) pos_min[i] = t.row >= 0 ? lo : -1;
    if (pos_max) pos_max[i] = hi;
    // the 16-bit copy of the positions the lanes read must say the same as the list
    if (t.row >= 0)
      for (int q = 0; q < 4; ++q)
        for (int u = 0; u < SW_RU; ++u) {
          const int n4 = t.n & ~3, e = std::max(std::min(q + 4 * u, n4 - 4 + q), 0);
          const unsigned w = (unsigned)c16[t.c16_off + 4 * q + (u >> 1)];
          if ((int)((w >> (16 * (u & 1))) & 0xffffu) != cpos[t.cpos_off + std::min(e, t.n - 1)]) return -5;
        }
  }
  return 0;
}

int qtos_set_heightfields(QtosPlanner *p, int n_maps, const double *height, int hnx, int hny,
                          double cell, double x0, double y0) {
  if (!p) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  if (p->d_height) {
    (void)hipFree(p->d_height);
    p->d_height = nullptr;
  }
  p->height_cnt = 0;
  p->height_pending = false;                               // (hipFree waited for the device: a copy into the old buffer is over)
  p->dp.height = nullptr;
  p->dp.n_maps = 0;
  if (n_maps <= 0 || !height) return 0;
  if (hnx < 1 || hny < 1 || !(cell > 0)) return -1;
  const size_t cnt = (size_t)n_maps * hnx * hny;
  HIPCHK(p, hipMalloc((void **)&p->d_height, cnt * sizeof(double)));
  HIPCHK(p, hipMemcpy(p->d_height, height, cnt * sizeof(double), hipMemcpyHostToDevice));
  p->height_cnt = cnt;
  p->dp.height = p->d_height;
  p->dp.n_maps = n_maps; p->dp.hnx = hnx; p->dp.hny = hny;
  p->dp.hcell = cell; p->dp.hx0 = x0; p->dp.hy0 = y0;
  return 0;
}

// The terrain from device memory.  Both directions are ordered here, since the caller cannot name the handle's streams: the copy
// waits for the end of the handle's last call (which may still read a kept buffer), and the handle's own stream -- every
// host-pointer entry point runs there -- waits for the copy; a solve submitted on a third stream waits in qtos_plan_batch_device.
int qtos_set_heightfields_device(QtosPlanner *p, int n_maps, const double *d_height, int hnx, int hny,
                                 double cell, double x0, double y0, void *stream) {
  if (!p) return -1;
  if (p->call_open || p->busy.load()) { p->err = "qtos_set_heightfields_device: a call is open (its kernels read the terrain)"; return -5; }
  if (n_maps <= 0) return qtos_set_heightfields(p, 0, nullptr, 0, 0, 1.0, 0.0, 0.0);
  if (!d_height || hnx < 1 || hny < 1 || !(cell > 0)) {
    p->err = "qtos_set_heightfields_device: d_height is not null, hnx and hny are >= 1, cell is > 0";
    return -1;
  }
  HIPCHK(p, hipSetDevice(p->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t cnt = (size_t)n_maps * hnx * hny;
  if (!p->d_height || p->height_cnt != cnt) {              // (a buffer of the same size is written again: no device-wide wait)
    if (p->d_height) (void)hipFree(p->d_height);
    p->d_height = nullptr;
    p->dp.height = nullptr;
    p->dp.n_maps = 0;
    p->height_cnt = 0;
    p->height_pending = false;
    HIPCHK(p, hipMalloc((void **)&p->d_height, cnt * sizeof(double)));
    p->height_cnt = cnt;
  }
  if (!p->ev_height) HIPCHK(p, hipEventCreateWithFlags(&p->ev_height, hipEventDisableTiming));
  // the last call's kernels, and whatever the host forms queued, are through with the buffer before it is written
  if (p->seq && p->last_stream != st) HIPCHK(p, hipStreamWaitEvent(st, p->lanes[0].ev[EV_CALL_END], 0));
  if (p->height_pending && p->height_stream != st) HIPCHK(p, hipStreamWaitEvent(st, p->ev_height, 0));   // (an earlier copy into the same buffer)
  HIPCHK(p, hipMemcpyAsync(p->d_height, d_height, cnt * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(p, hipEventRecord(p->ev_height, st));
  if (st != p->own_stream) HIPCHK(p, hipStreamWaitEvent(p->own_stream, p->ev_height, 0));
  p->height_stream = st;
  p->height_pending = true;
  p->dp.height = p->d_height;
  p->dp.n_maps = n_maps; p->dp.hnx = hnx; p->dp.hny = hny;
  p->dp.hcell = cell; p->dp.hx0 = x0; p->dp.hy0 = y0;
  return 0;
}

// results of a batch to the caller's buffers (one launch instead of four copies) and the running totals of
// qtos_plan_totals
// The counts of unfinished problems to the host: a store into mapped pinned memory by a one-wave kernel.  (A copy
// (hipMemcpyAsync) between two kernels of a stream makes the compute queue wait on the copy engine's signal; with more
// streams than hardware queues that wait holds up the other streams of the queue too: four sets of receding windows
// then ran one after the other.)
// The word carries the sequence number of the call that queued the launch: blind iterations a call queued beyond its end
// still store into their slots AFTER the next call of the handle has reset them (qtos_plan_submit), and a word of another
// call must read as "no counts yet", not as "nothing left to do" (call_schedule.hpp: pack_counts, read_counts).
__global__ void k_post_counts(const int *n_active, int *host_slot, unsigned seq) {
  // the two diagnostics first (earliest launch slot a problem sat out, launch slots with work), then both counts in ONE
  // eight-byte store: the host spins on that word (qtos_plan_poll) and must never see half of it
  if (threadIdx.x == 0) {
    const unsigned long long d = (unsigned long long)(unsigned)n_active[2] | ((unsigned long long)(unsigned)n_active[3] << 32);
    *(volatile unsigned long long *)(host_slot + SAT_OUT_AT) = d;
    __threadfence_system();
    *(volatile unsigned long long *)host_slot = pack_counts((unsigned)n_active[0], (unsigned)n_active[1], seq);
  }
  __threadfence_system();
}

// One launch slot of the call in flight, queued on its stream: the solve kernels the lane's progress names for it (c.ran[it]:
// KIND_KKT, KIND_CHORD), then k_step, then the counts to the host where it reads them.
//   informed  the counts of unfinished problems (n) and of problems flagged for a chord step (nc) in front of the slot are
//             known: kinds = the kernels with work; next to a factorisation of other problems the chord solve runs on the
//             side stream (the workgroups of the factorising kernel that belong to its problems leave at once and k_chord
//             gets their CUs: the batch pays max(k_kkt, k_chord), not the sum).
//   pattern   kinds = what this slot of the handle's last calls needed (QtosPlanner::pat), queued before any count of this
//             call has come back; a problem that waits for the other kernel sits the launch out (k_step).
//   blind     both kernels (qtos_set_speculation; each leaves at once for the problems that are not its own).
static int queue_iteration(QtosPlanner *p, QtosPlanner::Lane &c, int it) {
  const DevPlan &D = p->dp;
  const SlotLayout &L = p->slots;
  hipStream_t st = c.st;
  const int kinds = c.ran[it];
  const bool do_kkt = kinds & KIND_KKT, do_chord = (kinds & KIND_CHORD) != 0;
  const bool fork = do_kkt && do_chord;
  hipStream_t cs = fork ? c.side : st;
  if (fork) { HIPCHK(p, hipEventRecord(c.ev_fork, st)); HIPCHK(p, hipStreamWaitEvent(cs, c.ev_fork, 0)); }   // behind everything up to the previous k_step
  if (do_kkt) {
    if (p->per_kernel_events) HIPCHK(p, hipEventRecord(c.ev[L.ev(it, KKT_BEGIN)], st));
    hipLaunchKernelGGL(p->kkt_fn, dim3(c.B), dim3(p->kkt_threads), p->kkt_lds, st, D, c.W, c.B);
    if (p->per_kernel_events) HIPCHK(p, hipEventRecord(c.ev[L.ev(it, KKT_END)], st));
  }
  if (do_chord) {
    if (p->per_kernel_events) HIPCHK(p, hipEventRecord(c.ev[L.ev(it, CHORD_BEGIN)], cs));
    hipLaunchKernelGGL(p->chord_fn, dim3(c.B), dim3(KTC), chord_lds_bytes(p->S.n_stages, p->dp.sw_on ? p->dp.sw_steps : 0), cs, D, c.W, c.B);
    if (p->per_kernel_events) HIPCHK(p, hipEventRecord(c.ev[L.ev(it, CHORD_END)], cs));
  }
  if (fork) { HIPCHK(p, hipEventRecord(c.ev_join, cs)); HIPCHK(p, hipStreamWaitEvent(st, c.ev_join, 0)); }
  hipLaunchKernelGGL(k_step, dim3(c.B), dim3(ET), p->eval_lds, st, D, c.W, c.B, it, kinds);
  if (c.reads(it + 1)) hipLaunchKernelGGL(k_post_counts, dim3(1), dim3(64), 0, st, c.W.n_active, c.h_active_dev + L.counts_at(it + 1), p->seq);
  if (p->per_kernel_events) HIPCHK(p, hipEventRecord(c.ev[L.ev(it, SLOT_END)], st));
  return 0;
}

// A call that has ended, or failed on the way: the handle takes the next one (which opens the lanes it uses afresh).
static int close_call(QtosPlanner *p, int rc) {
  p->call_open = false; p->busy.store(0);
  return rc;
}

// The part [b0, b0 + B) of the planner's workspace and of the caller's buffers, as a workspace of its own (every array is
// indexed by the problem's number inside its launch).  Strides: the allocations in qtos_planner_create.
static DevWork work_slice(const QtosPlanner *p, const DevWork &w, int b0, int *n_active) {
  DevWork s = w;
  const size_t n = p->M.n_vars, m = p->M.n_cons, ns = p->M.n_sol, NS = p->S.n_stages, b = (size_t)b0;
  auto off = [&](auto *&ptr, size_t stride) { if (ptr) ptr += b * stride; };
  off(s.start, QTOS_START_DOUBLES); off(s.goal, 3); off(s.warm, n); off(s.map_id, 1);
  off(s.x, n); off(s.g, m); off(s.gt, m); off(s.s, m); off(s.zl, m); off(s.zu, m); off(s.ds, m); off(s.dzl, m); off(s.dzu, m);
  off(s.sig, m); off(s.w, m); off(s.panel, (size_t)p->dp.panel_stride); off(s.dx, ns); off(s.stream, (size_t)p->dp.stream_len);
  off(s.mu, 1); off(s.viol, 1); off(s.trace, ((size_t)p->dp.max_iter + 1) * 4); off(s.best_viol, 1); off(s.xbest, n);
  off(s.held, 1); off(s.best_it, 1); off(s.status, 1); off(s.iters, 1); off(s.done, 1);
  off(s.chord, 1); off(s.chord_run, 1); off(s.jam, 1); off(s.rhs, (size_t)p->S.n_unknowns); off(s.minv, NS * PIV * PIV);
  off(s.sol, NS * PIV); off(s.sol0, NS * PIV); off(s.dx0, ns); off(s.ur, m);
  off(s.nodes_out, n); off(s.viol_out, 1); off(s.status_out, 1); off(s.iters_out, 1);
  off(s.hist, ((size_t)p->dp.max_iter + 1) * HIST_COLS); off(s.rep, REP_COLS);
  s.n_active = n_active;
  return s;
}

// The launches of the call with workspace W on stream st, lane by lane.  The first failure ends it (the caller closes the call).
static int queue_call(QtosPlanner *p, int B, DevWork W, hipStream_t st) {
  if (hipSetDevice(p->device) != hipSuccess) return -2;
  if (p->height_pending) {                                 // a terrain copied in on another stream (qtos_set_heightfields_device)
    if (hipEventQuery(p->ev_height) == hipSuccess) p->height_pending = false;
    else if (st != p->height_stream && st != p->own_stream && hipStreamWaitEvent(st, p->ev_height, 0) != hipSuccess) return -2;
  }
  p->call_open = true; p->call_stream = st;
  p->seq = next_seq(p->seq);   // (blind iterations, whose late stores the number tells apart, are off by default: spec_cap 1)
  // the report is latched here for the whole call: without it the kernels see null pointers (no history, no k_report)
  if (!p->report) { W.hist = nullptr; W.rep = nullptr; }
  p->last_report = p->report; p->last_B = B;
  const DevPlan &D = p->dp;
  const SlotLayout &L = p->slots;
  const LaneSplit split(B, p->lane_chunk, (int)p->lanes.size());
  p->lanes_used = split.n_used;
  if (split.n_used > 1) HIPCHK(p, hipEventRecord(p->ev_in, st));
  const LaunchPattern *pattern = p->pattern.serving(split.n_used, p->spec_cap);   // (null: this call does not follow it)
  for (int j = 0; j < split.n_used; ++j) {
    QtosPlanner::Lane &c = p->lanes[j];
    c.b0 = split.first(j); c.B = split.size(j); c.spins = 0;
    // the slots queued at once: the pattern's prefix, or as many blind iterations as the previous call of this handle needed (its
    // slowest problem; qtos_set_speculation, 1 by default: the first iteration).  A batch that needs more is continued by
    // qtos_plan_poll from the counts the iterations send back; blind launches behind the end find every problem done.
    c.begin(pattern, blind_slots(p->last_iters, p->spec_cap, D.max_iter), L);
    c.st = j == 0 ? st : c.own;
    c.W = work_slice(p, W, c.b0, c.d_n_active);
    if (j > 0) HIPCHK(p, hipStreamWaitEvent(c.st, p->ev_in, 0));
    std::memset(c.h_active, 0xff, L.count_ints() * sizeof(int));   // no counts yet (late stores of an earlier call carry another sequence number)
    HIPCHK(p, hipMemsetAsync(c.W.n_active, 0, 4 * sizeof(int), c.st));
    HIPCHK(p, hipEventRecord(c.ev[EV_CALL_BEGIN], c.st));
    hipLaunchKernelGGL(k_start, dim3(c.B), dim3(ET), p->eval_lds, c.st, D, c.W, c.B);
    // (a call that follows the pattern reads no counts in front of the pattern's last slot and posts none)
    if (c.reads(0)) hipLaunchKernelGGL(k_post_counts, dim3(1), dim3(64), 0, c.st, c.W.n_active, c.h_active_dev + L.counts_at(0), p->seq);
    if (p->per_kernel_events) HIPCHK(p, hipEventRecord(c.ev[L.ev_start_end()], c.st));
    for (int it = 0; it < c.spec; ++it)
      if (int rc = queue_iteration(p, c, it)) return rc;
  }
  if (split.n_used == 1 && hipEventRecord(p->lanes[0].ev[EV_CALL_END], st) != hipSuccess) return -2;
  p->last_stream = st;
  return 0;
}

int qtos_plan_submit(QtosPlanner *p, int B, const double *d_start, const double *d_goal,
                     const int *d_map_id, const double *d_warm, double *d_nodes_out,
                     int *d_status_out, int *d_iters_out, double *d_viol_out, void *stream_) {
  if (!p || B < 1 || B > p->max_batch || !d_start || !d_goal || !d_nodes_out) return -1;
  int expected = 0;
  if (!p->busy.compare_exchange_strong(expected, 1)) { p->err = "the planner handle already serves a call (one call per handle at a time)"; return -5; }
  DevWork W = p->wk;
  W.start = d_start; W.goal = d_goal; W.map_id = d_map_id; W.warm = d_warm;
  // (the kernel that finishes a problem writes its result: kernels.hpp export_problem)
  W.nodes_out = d_nodes_out; W.status_out = d_status_out; W.iters_out = d_iters_out; W.viol_out = d_viol_out;
  W.totals = (unsigned long long *)p->d_totals;
  const int rc = queue_call(p, B, W, (hipStream_t)stream_);
  return rc ? close_call(p, rc) : 0;
}

// hipSetDevice once per poll, and only in front of a launch: in a spin loop of several host threads it is a lock fight.
static int launch_device(QtosPlanner *p, bool *device_set) {
  if (!*device_set) HIPCHK(p, hipSetDevice(p->device));
  *device_set = true;
  return 0;
}

// One lane as far as the counts that have arrived allow.  It is through (c.open goes) when every problem of the part has handed
// its result over (export_problem; a problem out of iterations counts as finished).
static int advance_lane(QtosPlanner *p, QtosPlanner::Lane &c, bool *device_set) {
  for (int slot = 0;;) {
    const LaneProgress::Act act = c.next(c.h_active, p->slots, p->seq, &slot);
    if (act == LaneProgress::QUEUE) {
      if (int rc = launch_device(p, device_set)) return rc;
      if (int rc = queue_iteration(p, c, slot)) return rc;
      if (p->lanes_used == 1) HIPCHK(p, hipEventRecord(c.ev[EV_CALL_END], c.st));   // (the end-of-call event sits behind the last launch)
    } else if (act != LaneProgress::STEP) {
      // Waiting: the word itself says when the counts are there (k_post_counts stores into mapped host memory) -- an event query
      // on top of it is a driver call and waits for the end-of-kernel signal of the command processor.  A failed launch never
      // fills the slot: look at the stream now and then.
      if (act == LaneProgress::WAIT && (++c.spins & 0xfffff) == 0) {
        const hipError_t q = hipStreamQuery(c.st);
        if (q != hipSuccess && q != hipErrorNotReady) { p->err = std::string("hipStreamQuery: ") + hipGetErrorString(q); return -2; }
      }
      return 0;
    }
  }
}

// The lanes of the open call as far as they get; n_open: those that are not through.
static int advance_call(QtosPlanner *p, int *n_open) {
  bool device_set = false;
  for (int j = 0; j < p->lanes_used; ++j) {
    QtosPlanner::Lane &c = p->lanes[j];
    if (!c.open) continue;
    if (int rc = advance_lane(p, c, &device_set)) return rc;
    if (c.open) { ++*n_open; continue; }
    if ((c.W.rep || j > 0) && launch_device(p, &device_set)) return -2;
    if (c.W.rep) {   // report on: the final measures of the lane's problems, behind the lane's last launch and its end event
      hipLaunchKernelGGL(k_report, dim3(c.B), dim3(ET), p->eval_lds, c.st, p->dp, c.W, c.B);
      if (hipGetLastError() != hipSuccess) return -2;
    }
    // the caller's stream waits for the part that ran beside it
    if (j > 0 && (hipEventRecord(c.ev_done, c.st) != hipSuccess || hipStreamWaitEvent(p->call_stream, c.ev_done, 0) != hipSuccess)) return -2;
  }
  if (*n_open == 0 && p->lanes_used > 1)   // end of the call: behind every part
    if (launch_device(p, &device_set) || hipEventRecord(p->lanes[0].ev[EV_CALL_END], p->call_stream) != hipSuccess) return -2;
  return 0;
}

int qtos_plan_poll(QtosPlanner *p, int *done) {
  if (!p || !done) return -1;
  *done = 0;
  if (!p->call_open) { *done = 1; return 0; }
  int n_open = 0;
  if (int rc = advance_call(p, &n_open)) return close_call(p, rc);
  if (n_open) return 0;
  p->last_iters = 0;
  for (int j = 0; j < p->lanes_used; ++j) p->last_iters = std::max(p->last_iters, p->lanes[j].last_launches);
  // the launch pattern of the next call, from what this one's slots ran
  if (p->lanes_used == 1) p->pattern.update(p->lanes[0].ran, p->lanes[0].last_launches, p->lanes[0].sat_out);
  *done = 1;
  return close_call(p, 0);
}

int qtos_plan_wait(QtosPlanner *p) {
  if (!p) return -1;
  int done = 0;
  while (!done)
    if (int rc = qtos_plan_poll(p, &done)) return rc;
  return 0;
}

int qtos_plan_batch_device(QtosPlanner *p, int B, const double *d_start, const double *d_goal,
                           const int *d_map_id, const double *d_warm, double *d_nodes_out,
                           int *d_status_out, int *d_iters_out, double *d_viol_out, void *stream_) {
  if (int rc = qtos_plan_submit(p, B, d_start, d_goal, d_map_id, d_warm, d_nodes_out, d_status_out, d_iters_out, d_viol_out, stream_)) return rc;
  return qtos_plan_wait(p);
}

int qtos_set_speculation(QtosPlanner *p, int max_blind_iterations) {
  if (!p || max_blind_iterations < 0) return -1;
  p->spec_cap = max_blind_iterations;
  return 0;
}

int qtos_plan_totals(QtosPlanner *p, long long *converged, long long *iterations, int reset) {
  if (!p) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  long long h[2] = {0, 0};
  // on the planner's own stream, behind the end event of the last call (the caller's stream may be gone by now)
  if (p->call_open) HIPCHK(p, qtos_plan_wait(p) ? hipErrorUnknown : hipSuccess);
  HIPCHK(p, hipStreamWaitEvent(p->own_stream, p->lanes[0].ev[EV_CALL_END], 0));
  HIPCHK(p, hipMemcpyAsync(h, p->d_totals, sizeof(h), hipMemcpyDeviceToHost, p->own_stream));
  if (reset) HIPCHK(p, hipMemsetAsync(p->d_totals, 0, sizeof(h), p->own_stream));
  HIPCHK(p, hipStreamSynchronize(p->own_stream));
  if (converged) *converged = h[0];
  if (iterations) *iterations = h[1];
  return 0;
}

int qtos_plan_batch(QtosPlanner *p, int B, const double *start, const double *goal, const int *map_id,
                    const double *warm, double *nodes_out, int *status_out, int *iters_out, double *viol_out) {
  if (!p || B < 1 || B > p->max_batch || !start || !goal || !nodes_out) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t n = p->M.n_vars;
  if (map_id)   // (the kernels clamp too; a wrong id is the caller's bug and is reported)
    for (int b = 0; b < B; ++b)
      if (map_id[b] < 0 || map_id[b] >= std::max(p->dp.n_maps, 1)) { p->err = "map_id out of range"; return -1; }
  hipStream_t st = p->own_stream;   // stream-scoped: no device-wide synchronisation
  HIPCHK(p, hipMemcpyAsync(p->d_start, start, (size_t)B * QTOS_START_DOUBLES * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(p, hipMemcpyAsync(p->d_goal, goal, (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  if (map_id) HIPCHK(p, hipMemcpyAsync(p->d_map, map_id, B * sizeof(int), hipMemcpyHostToDevice, st));
  if (warm) HIPCHK(p, hipMemcpyAsync(p->d_warm, warm, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, st));
  int rc = qtos_plan_batch_device(p, B, p->d_start, p->d_goal, map_id ? p->d_map : nullptr,
                                  warm ? p->d_warm : nullptr, p->d_nodes, nullptr, nullptr, nullptr, (void *)st);
  if (rc) return rc;
  HIPCHK(p, hipMemcpyAsync(nodes_out, p->d_nodes, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (status_out) HIPCHK(p, hipMemcpyAsync(status_out, p->wk.status, B * sizeof(int), hipMemcpyDeviceToHost, st));
  if (iters_out) HIPCHK(p, hipMemcpyAsync(iters_out, p->wk.iters, B * sizeof(int), hipMemcpyDeviceToHost, st));
  if (viol_out) HIPCHK(p, hipMemcpyAsync(viol_out, p->wk.viol, B * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(p, hipStreamSynchronize(st));
  return 0;
}

// Timing of the last call from the HIP events of its lanes.  The events are there once the call's end event is.
static int timing_events(QtosPlanner *p) {
  if (!p->per_kernel_events) { p->err = "per-kernel events are off (qtos_set_kernel_events)"; return -1; }
  HIPCHK(p, hipSetDevice(p->device));
  HIPCHK(p, hipEventSynchronize(p->lanes[0].ev[EV_CALL_END]));
  return 0;
}
// Launches of one solve kernel (kind: KIND_KKT between KKT_BEGIN and KKT_END, KIND_CHORD between CHORD_BEGIN and CHORD_END) and
// their seconds, summed over the lanes.
static int kind_timing(QtosPlanner *p, int kind, SlotEvent begin, SlotEvent end, double *seconds, int *launches) {
  if (int rc = timing_events(p)) return rc;
  double t = 0;
  int nl = 0;
  for (int j = 0; j < p->lanes_used; ++j) {
    const QtosPlanner::Lane &L = p->lanes[j];
    for (int i = 0; i < L.last_launches; ++i) {
      if (!(L.ran[i] & kind)) continue;
      float ms = 0;
      HIPCHK(p, hipEventElapsedTime(&ms, L.ev[p->slots.ev(i, begin)], L.ev[p->slots.ev(i, end)]));
      t += ms * 1e-3;
      ++nl;
    }
  }
  if (seconds) *seconds = t;
  if (launches) *launches = nl;
  return 0;
}

// total = first kernel of lane 0 to the end of the call, iterations = the slowest lane's.
int qtos_last_timing(QtosPlanner *p, double *kkt_seconds, int *kkt_launches, double *total_seconds, int *iterations) {
  if (!p) return -1;
  if (int rc = kind_timing(p, KIND_KKT, KKT_BEGIN, KKT_END, kkt_seconds, kkt_launches)) return rc;
  float tot = 0;
  HIPCHK(p, hipEventElapsedTime(&tot, p->lanes[0].ev[EV_CALL_BEGIN], p->lanes[0].ev[EV_CALL_END]));
  if (total_seconds) *total_seconds = tot * 1e-3;
  if (iterations) *iterations = p->last_iters;
  return 0;
}

int qtos_last_timing_chord(QtosPlanner *p, double *chord_seconds, int *chord_launches) {
  return p ? kind_timing(p, KIND_CHORD, CHORD_BEGIN, CHORD_END, chord_seconds, chord_launches) : -1;
}

// Where the time of the last call went, from the same events (lane 0; one lane per call is what bench.py times):
//   out[0] first kernel -> end of the call            out[1] memset + k_start (+ its counts)
//   out[2] solve kernels (a slot's factorisation and chord solve side by side count once)
//   out[3] k_step + counts of every slot (from the end of the slot's solve to its last event)
//   out[4] GAPS: from a slot's last event to the first event of the next slot's solve -- the host reading the counts and
//          launching (zero between slots queued at submit time) -- plus whatever lies between the last slot and the end event
//   out[5] launch slots with work, out[6] slots queued at submit time (pattern / blind), out[7] launches that waited for the host
//   out[8] calls of the handle that followed a pattern so far, out[9] of those, calls in which a problem sat a slot out
//   n_out >= 14: out[10] seconds / out[11] launches of the factorising kernel, out[12] / out[13] of k_chord (qtos_last_timing's and
//   qtos_last_timing_chord's numbers: one call instead of three in a timed loop)
int qtos_last_timing_detail(QtosPlanner *p, double *out, int n_out) {
  if (!p || !out || n_out < 10) return -1;
  if (int rc = timing_events(p)) return rc;
  const QtosPlanner::Lane &L = p->lanes[0];
  auto ms = [&](hipEvent_t a, hipEvent_t b, double *d) { float t = 0; hipError_t e = hipEventElapsedTime(&t, a, b); *d = t * 1e-3; return e; };
  double tot = 0, start = 0, solve = 0, step = 0, gaps = 0, kkt_s = 0, chord_s = 0;
  int kkt_n = 0, chord_n = 0;
  HIPCHK(p, ms(L.ev[EV_CALL_BEGIN], L.ev[EV_CALL_END], &tot));
  HIPCHK(p, ms(L.ev[EV_CALL_BEGIN], L.ev[p->slots.ev_start_end()], &start));
  hipEvent_t prev = L.ev[p->slots.ev_start_end()];
  for (int i = 0; i < L.enq; ++i) {
    const bool kkt = L.ran[i] & KIND_KKT, chord = (L.ran[i] & KIND_CHORD) != 0;
    auto ev = [&](SlotEvent e) { return L.ev[p->slots.ev(i, e)]; };
    if (!kkt && !chord && i >= L.last_launches) continue;   // (queued behind the end: nothing ran)
    hipEvent_t b0 = kkt ? ev(KKT_BEGIN) : (chord ? ev(CHORD_BEGIN) : nullptr);
    double g = 0, sk = 0, sc = 0, st = 0;
    if (b0) {
      HIPCHK(p, ms(prev, b0, &g));
      if (kkt) HIPCHK(p, ms(b0, ev(KKT_END), &sk));
      if (chord) HIPCHK(p, ms(b0, ev(CHORD_END), &sc));
      if (i < L.last_launches) {
        if (kkt) { kkt_s += sk; ++kkt_n; }
        if (chord) { double own = sc; if (kkt) HIPCHK(p, ms(ev(CHORD_BEGIN), ev(CHORD_END), &own)); chord_s += own; ++chord_n; }
      }
      const double sv = std::max(sk, sc);
      double whole = 0;
      HIPCHK(p, ms(b0, ev(SLOT_END), &whole));
      st = std::max(0.0, whole - sv);
      gaps += std::max(0.0, g); solve += sv; step += st;
    } else {
      HIPCHK(p, ms(prev, ev(SLOT_END), &st));
      step += st;
    }
    prev = ev(SLOT_END);
  }
  gaps += std::max(0.0, tot - start - solve - step - gaps);
  out[0] = tot; out[1] = start; out[2] = solve; out[3] = step; out[4] = gaps;
  out[5] = L.last_launches; out[6] = L.spec; out[7] = L.n_informed;
  out[8] = (double)p->pattern.calls; out[9] = (double)p->pattern.misses;
  if (n_out >= 14) { out[10] = kkt_s; out[11] = kkt_n; out[12] = chord_s; out[13] = chord_n; }
  return 0;
}

static_assert(HIST_COLS == QTOS_HIST_COLS && H_INF_DU == QTOS_H_INF_DU && H_KIND == QTOS_H_KIND, "history layout: kernels.hpp and the header");

int qtos_set_report(QtosPlanner *p, int on) {
  if (!p) return -1;
  if (p->call_open || p->busy.load()) { p->err = "qtos_set_report: a call is open (the flag is latched per call at submit)"; return -5; }
  p->report = on != 0;
  return 0;
}

int qtos_plan_report(QtosPlanner *p, int b, QtosReport *out, double *rows, int max_rows) {
  if (!p || !out || b < 0 || (rows && max_rows < 0)) return -1;
  if (!p->last_report || b >= p->last_B) { p->err = "qtos_plan_report: the last call ran without the report, or b is outside it"; return -6; }
  if (p->call_open) return -5;
  HIPCHK(p, hipSetDevice(p->device));
  HIPCHK(p, hipStreamSynchronize(p->last_stream));   // (k_report runs behind the call's end event)
  const int stride = p->M.P.max_iter + 1;
  int st = 0, it = 0;
  double rep[REP_COLS];
  std::vector<double> h((size_t)stride * HIST_COLS);
  HIPCHK(p, hipMemcpy(&st, p->wk.status + b, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(p, hipMemcpy(&it, p->wk.iters + b, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(p, hipMemcpy(rep, p->wk.rep + (size_t)b * REP_COLS, sizeof(rep), hipMemcpyDeviceToHost));
  HIPCHK(p, hipMemcpy(h.data(), p->wk.hist + (size_t)b * stride * HIST_COLS, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  const int n_rows = std::min(it + 1, stride);
  std::memset(out, 0, sizeof(*out));
  out->status = st; out->iterations = it; out->n_rows = n_rows;
  out->n_con_evals = 1; out->n_jac_evals = 1;
  for (int i = 1; i < n_rows; ++i) {
    const double *r = h.data() + (size_t)i * HIST_COLS;
    out->n_con_evals += (int)r[H_LS];
    if (r[H_KIND] == 0) out->n_factorizations++; else out->n_chord_solves++;
    if (i + 1 < n_rows) out->n_jac_evals++;   // (the step that finished the solve needs no linearisation)
  }
  out->constraint_violation = rep[R_VIOL]; out->dual_infeasibility = rep[R_INF_DU];
  out->complementarity = rep[R_COMPL]; out->nlp_error = rep[R_ERR];
  if (rows && max_rows > 0) std::memcpy(rows, h.data(), (size_t)std::min(n_rows, max_rows) * HIST_COLS * sizeof(double));
  return n_rows;
}

int qtos_analyze_counts(const QtosParams *params, long long *counts, int n) {
  if (!params || !counts || n < 0) return -1;
  QtosParams full = *params;
  full.reduce_base = 0; full.reduce_swing = 0;
  HostModel M;
  if (M.build(full)) { fprintf(stderr, "qtos: %s\n", M.err.c_str()); return -1; }
  long long nz[2] = {0, 0};
  for (const Block &blk : M.blocks)
    for (int r = 0; r < blk.m; ++r) {
      const int row = blk.row0 + r, k = M.con_lo[row] == M.con_hi[row] ? 0 : 1;
      for (int a = 0; a < blk.n; ++a) nz[k] += M.is_free(M.block_cols[blk.col_off + a]) ? 1 : 0;
    }
  const int k = std::min(n, 2);
  for (int i = 0; i < k; ++i) counts[i] = nz[i];
  return k;
}

int qtos_set_kernel_events(QtosPlanner *p, int on) {
  if (!p) return -1;
  p->per_kernel_events = on != 0;
  return 0;
}

int qtos_set_pattern_speculation(QtosPlanner *p, int on) {
  if (!p) return -1;
  p->pattern.on = on != 0;
  if (!on) p->pattern.clear();
  return 0;
}

int qtos_env(const QtosPlanner *p, char *buf, int n) {
  if (!p || !buf || n < 1) return -1;
  const std::string d = p->env.describe();
  snprintf(buf, (size_t)n, "%s", d.c_str());
  return (int)d.size();
}

#include "window_api.hpp"

int qtos_set_init_table(QtosPlanner *p, int ndx, const double *dx, int ndy, const double *dy, const double *nodes) {
  if (!p) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  for (void *q : {(void *)p->d_table, (void *)p->d_tab_dx, (void *)p->d_tab_dy})
    if (q) (void)hipFree(q);
  p->d_table = p->d_tab_dx = p->d_tab_dy = nullptr;
  p->dp.table = p->dp.tab_dx = p->dp.tab_dy = nullptr;
  p->dp.tab_ndx = p->dp.tab_ndy = 0;
  if (ndx <= 0 || ndy <= 0 || !dx || !dy || !nodes) return 0;
  for (int i = 1; i < ndx; ++i) if (!(dx[i] > dx[i - 1])) return -1;
  for (int j = 1; j < ndy; ++j) if (!(dy[j] > dy[j - 1])) return -1;
  const size_t cnt = (size_t)ndx * ndy * p->M.n_vars;
  HIPCHK(p, hipMalloc((void **)&p->d_table, cnt * sizeof(double)));
  HIPCHK(p, hipMalloc((void **)&p->d_tab_dx, ndx * sizeof(double)));
  HIPCHK(p, hipMalloc((void **)&p->d_tab_dy, ndy * sizeof(double)));
  HIPCHK(p, hipMemcpy(p->d_table, nodes, cnt * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(p, hipMemcpy(p->d_tab_dx, dx, ndx * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(p, hipMemcpy(p->d_tab_dy, dy, ndy * sizeof(double), hipMemcpyHostToDevice));
  p->dp.table = p->d_table; p->dp.tab_dx = p->d_tab_dx; p->dp.tab_dy = p->d_tab_dy;
  p->dp.tab_ndx = ndx; p->dp.tab_ndy = ndy;
  return 0;
}

// ---- introspection -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_debug_guess(DevPlan P, DevWork W, int B, double *out) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const double *st = W.start + (size_t)b * QTOS_START_DOUBLES, *gl = W.goal + (size_t)b * 3;
  const int map = W.map_id ? W.map_id[b] : 0;
  const TableCell tc = table_cell(P, st, gl);
  for (int v = threadIdx.x; v < P.n_vars; v += blockDim.x) out[(size_t)b * P.n_vars + v] = initial_value(P, W, b, v, st, gl, map, tc);
  __syncthreads();
  double *y = out + (size_t)b * P.n_vars;
  for (int i = threadIdx.x; i < P.n_psw; i += blockDim.x)   // (reduced swings: k_start places the mid nodes on the swing rule)
    y[P.psw_var[i]] = fma(P.psw_w[2 * i], y[P.psw_src[2 * i]], P.psw_w[2 * i + 1] * y[P.psw_src[2 * i + 1]]);
}

// reduced base: what given nodes become when a solve starts from them (k_start's projection onto the coefficients' space)
__global__ __launch_bounds__(256) void k_project_nodes(DevPlan P, const double *in, double *out, int B) {
  extern __shared__ double cf[];
  const int b = blockIdx.x, n = P.n_vars;
  if (b >= B) return;
  const double *x = in + (size_t)b * n;
  double *y = out + (size_t)b * n;
  for (int v = threadIdx.x; v < n; v += blockDim.x) y[v] = x[v];
  for (int i = threadIdx.x; i < P.n_psw; i += blockDim.x)   // (reduced swings: mid nodes onto the swing rule; their sources are footholds)
    y[P.psw_var[i]] = fma(P.psw_w[2 * i], x[P.psw_src[2 * i]], P.psw_w[2 * i + 1] * x[P.psw_src[2 * i + 1]]);
  for (int c = threadIdx.x; c < P.n_coef; c += blockDim.x) {
    double acc = 0.0;
    for (int a = 0; a < 4; ++a) acc = fma(P.pc_w[4 * c + a], x[P.pc_var[4 * c + a]], acc);
    cf[c] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < P.n_pz; i += blockDim.x) {
    double acc = 0.0;
    for (int a = 0; a < 4; ++a) acc = fma(P.pz_w[4 * i + a], cf[P.pz_col[4 * i + a]], acc);
    y[P.pz_var[i]] = acc;
  }
}

int qtos_project_nodes(QtosPlanner *p, int B, const double *nodes, double *nodes_out) {
  if (!p || B < 1 || B > p->max_batch || !nodes || !nodes_out) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t bytes = (size_t)B * p->M.n_vars * sizeof(double);
  HIPCHK(p, hipMemcpy(p->d_warm, nodes, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_project_nodes, dim3(B), dim3(256), sizeof(double) * std::max(p->dp.n_coef, 1), 0, p->dp, p->d_warm, p->d_nodes, B);
  HIPCHK(p, hipDeviceSynchronize());
  HIPCHK(p, hipMemcpy(nodes_out, p->d_nodes, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int qtos_debug_initial_guess(QtosPlanner *p, int B, const double *start, const double *goal, const int *map_id, double *nodes_out) {
  if (!p || B < 1 || B > p->max_batch || !start || !goal || !nodes_out) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  HIPCHK(p, hipMemcpy(p->d_start, start, (size_t)B * QTOS_START_DOUBLES * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(p, hipMemcpy(p->d_goal, goal, (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice));
  if (map_id) HIPCHK(p, hipMemcpy(p->d_map, map_id, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
  DevWork W = p->wk;
  W.start = p->d_start; W.goal = p->d_goal; W.map_id = map_id ? p->d_map : nullptr; W.warm = nullptr;
  hipLaunchKernelGGL(k_debug_guess, dim3(B), dim3(256), 0, 0, p->dp, W, B, p->d_nodes);
  HIPCHK(p, hipDeviceSynchronize());
  HIPCHK(p, hipMemcpy(nodes_out, p->d_nodes, (size_t)B * p->M.n_vars * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

__global__ __launch_bounds__(256) void k_debug_eval(DevPlan P, DevWork W, int B) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const int n = P.n_vars, m = P.n_cons;
  double *x = W.x + (size_t)b * n, *g = W.g + (size_t)b * m;
  const double *st = W.start + (size_t)b * QTOS_START_DOUBLES, *gl = W.goal + (size_t)b * 3;
  for (int v = threadIdx.x; v < n; v += blockDim.x) {
    const InitDesc I = P.init[v];
    x[v] = I.fix_src >= 0 ? (I.fix_src < 24 ? st[I.fix_src] : (I.fix_src < 26 ? gl[I.fix_src - 24] : 0.0))
                          : W.warm[(size_t)b * n + v];
  }
  __syncthreads();
  extern __shared__ double evl[];
  eval_all<true>(P, W.map_id ? W.map_id[b] : 0, x, g, W.stream + (size_t)b * P.stream_len, evl);
  if (threadIdx.x == 0) W.done[b] = 0;
}

__global__ __launch_bounds__(256) void k_debug_pack(DevPlan P, DevWork W, int B) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const size_t m = P.n_cons;
  const double *g = W.g + b * m, *sig = W.sig + b * m, *w = W.w + b * m;
  double *stream = W.stream + (size_t)b * P.stream_len;
  for (int r = threadIdx.x; r < P.n_cons; r += blockDim.x) {
    if (P.row_kind[r] == 1) stream[P.rhs_pos[r]] = -g[r];
    if (P.row_kind[r] == 2) { stream[P.sig_pos[r]] = sig[r]; stream[P.w_pos[r]] = w[r]; }
  }
}

// reduced base: the step of the base node values from the step of the coefficients (what k_step does at its start), for
// the entry points that hand dx out
__global__ __launch_bounds__(256) void k_recover_dx(DevPlan P, DevWork W, int B) {
  const int b = blockIdx.x;
  if (b >= B) return;
  double *dx = W.dx + (size_t)b * P.n_sol;
  for (int i = threadIdx.x; i < P.n_rec; i += blockDim.x) {
    double acc = 0.0;
    for (int a = 0; a < 4; ++a) {
      const int col = P.rec_col[4 * i + a];
      if (col >= 0) acc = fma(P.rec_w[4 * i + a], dx[col], acc);
    }
    dx[P.rec_var[i]] = acc;
  }
}
// dx (node space, B x n_vars) of the last debug solve to the host
static int copy_dx_out(QtosPlanner *p, const DevWork &W, int B, double *dx_out) {
  if (p->dp.n_rec) hipLaunchKernelGGL(k_recover_dx, dim3(B), dim3(256), 0, 0, p->dp, W, B);
  HIPCHK(p, hipDeviceSynchronize());
  HIPCHK(p, hipMemcpy2D(dx_out, p->M.n_vars * sizeof(double), W.dx, p->M.n_sol * sizeof(double), p->M.n_vars * sizeof(double), B, hipMemcpyDeviceToHost));
  return 0;
}

static int debug_upload(QtosPlanner *p, int B, const double *start, const double *goal, const int *map_id, const double *nodes, DevWork *W) {
  if (!p || B < 1 || B > p->max_batch || !start || !goal || !nodes) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t n = p->M.n_vars;
  HIPCHK(p, hipMemcpy(p->d_start, start, (size_t)B * QTOS_START_DOUBLES * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(p, hipMemcpy(p->d_goal, goal, (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice));
  if (map_id) HIPCHK(p, hipMemcpy(p->d_map, map_id, B * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(p, hipMemcpy(p->d_warm, nodes, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice));
  *W = p->wk;
  W->start = p->d_start; W->goal = p->d_goal; W->map_id = map_id ? p->d_map : nullptr; W->warm = p->d_warm;
  hipLaunchKernelGGL(k_debug_eval, dim3(B), dim3(256), p->eval_lds, 0, p->dp, *W, B);
  HIPCHK(p, hipDeviceSynchronize());
  return 0;
}

int qtos_debug_eval(QtosPlanner *p, int B, const double *start, const double *goal, const int *map_id,
                    const double *nodes, double *g_out, double *J_out) {
  if (J_out && p && p->M.reduce_base) { p->err = "qtos_debug_eval: the Jacobian in node space is not formed with reduce_base (create the planner without it)"; return -1; }
  DevWork W;
  int rc = debug_upload(p, B, start, goal, map_id, nodes, &W);
  if (rc) return rc;
  const HostModel &M = p->M;
  const size_t n = M.n_vars, m = M.n_cons;
  if (g_out) HIPCHK(p, hipMemcpy(g_out, W.g, (size_t)B * m * sizeof(double), hipMemcpyDeviceToHost));
  if (J_out) {
    const size_t SL = p->S.pack_src.size();
    std::vector<double> G((size_t)B * SL);
    HIPCHK(p, hipMemcpy(G.data(), W.stream, G.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::memset(J_out, 0, (size_t)B * m * n * sizeof(double));
    for (int b = 0; b < B; ++b)
      for (const Block &blk : M.blocks)
        for (int r = 0; r < blk.m; ++r)
          for (int a = 0; a < blk.n; ++a) {
            double v;
            if (blk.gstatic) v = M.g_static[blk.goff + r * blk.n + a];
            else if (blk.kind == 1) v = G[(size_t)b * SL + blk.goff + r * blk.n + a];
            else v = G[(size_t)b * SL + p->S.eq_pos[blk.goff + r * blk.n + a]];
            J_out[((size_t)b * m + blk.row0 + r) * n + M.block_cols[blk.col_off + a]] = v;
          }
  }
  return 0;
}

int qtos_debug_newton(QtosPlanner *p, int B, const double *start, const double *goal, const int *map_id,
                      const double *nodes, const double *sig, const double *w, double *dx_out) {
  DevWork W;
  int rc = debug_upload(p, B, start, goal, map_id, nodes, &W);
  if (rc) return rc;
  const size_t n = p->M.n_vars, m = p->M.n_cons;
  HIPCHK(p, hipMemcpy(W.sig, sig, (size_t)B * m * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(p, hipMemcpy(W.w, w, (size_t)B * m * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_pack, dim3(B), dim3(256), 0, 0, p->dp, W, B);
  hipLaunchKernelGGL(p->kkt_fn, dim3(B), dim3(p->kkt_threads), p->kkt_lds, 0, p->dp, W, B);
  HIPCHK(p, hipDeviceSynchronize());
  if (int rc = copy_dx_out(p, W, B, dx_out)) return rc;
  return 0;
}

// right-hand side of the KKT system from the state debug_upload / k_debug_pack left behind (k_step's formula)
__global__ __launch_bounds__(256) void k_debug_rhs(DevPlan P, DevWork W, int B) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const size_t m = P.n_cons;
  const double *g = W.g + b * m, *wr = W.w + b * m, *Gs = W.stream + (size_t)b * P.stream_len;
  double *rhs = W.rhs + (size_t)b * P.n_unknowns;
  for (int p = threadIdx.x; p < P.n_unknowns; p += blockDim.x) {
    const int t0 = P.rhs_ptr[p], t1 = P.rhs_ptr[p + 1];
    double acc = 0.0;
    if (t1 - t0 == 1 && P.rhs_gpos[t0] < 0) acc = -g[P.rhs_row[t0]];
    else
      for (int t = t0; t < t1; ++t) acc = fma(-Gs[P.rhs_gpos[t]], wr[P.rhs_row[t]], acc);
    rhs[p] = acc;
  }
  if (threadIdx.x == 0) { W.chord[b] = 1; atomicAdd(W.n_active + 1, 1); }
}
__global__ void k_debug_flag_chord(DevWork W, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) { W.chord[b] = 1; atomicAdd(W.n_active + 1, 1); }
}
__global__ void k_debug_unchord(DevWork W, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) W.chord[b] = 0;
  if (b == 0) W.n_active[1] = 0;
}

/* the same solve as qtos_debug_newton once more, this time by k_chord: the factorisation the preceding
 * qtos_debug_newton call left behind + the right-hand side in elimination order.  dx_out: B x n_vars */
int qtos_debug_chord(QtosPlanner *p, int B, double *dx_out) {
  if (!p || B < 1 || B > p->max_batch || !dx_out || !p->chord_fn) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  DevWork W = p->wk;
  hipLaunchKernelGGL(k_debug_rhs, dim3(B), dim3(256), 0, 0, p->dp, W, B);
  hipLaunchKernelGGL(p->chord_fn, dim3(B), dim3(KTC), chord_lds_bytes(p->S.n_stages, p->dp.sw_on ? p->dp.sw_steps : 0), 0, p->dp, W, B);
  hipLaunchKernelGGL(k_debug_unchord, dim3((B + 63) / 64), dim3(64), 0, 0, W, B);
  HIPCHK(p, hipDeviceSynchronize());
  if (int rc = copy_dx_out(p, W, B, dx_out)) return rc;
  return 0;
}

/* A-posteriori check of the system the preceding qtos_debug_newton call solved: res_rel_out[b] = max |b - K x| / max |b|
 * with K applied from the problem's stream (k_residual: no use of the factorisation).  refine != 0: one step of
 * iterative refinement through the stored factorisation first -- r = b - K x, K e = r by k_chord, x += e -- and the
 * residual of the refined solution; dx_out (B x n_vars, may be NULL) receives the solution. */
int qtos_debug_residual(QtosPlanner *p, int B, int refine, double *dx_out, double *res_rel_out) {
  if (!p || B < 1 || B > p->max_batch || !res_rel_out) return -1;
  if (refine && !p->chord_fn) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  DevWork W = p->wk;
  double *d_out = nullptr;
  HIPCHK(p, hipMalloc((void **)&d_out, B * sizeof(double)));
  if (refine) {
    hipLaunchKernelGGL(k_residual, dim3(B), dim3(512), 0, 0, p->dp, W, B, (double *)nullptr, 1);   // r -> W.rhs, x remembered
    hipLaunchKernelGGL(k_debug_flag_chord, dim3((B + 63) / 64), dim3(64), 0, 0, W, B);
    hipLaunchKernelGGL(p->chord_fn, dim3(B), dim3(KTC), chord_lds_bytes(p->S.n_stages, p->dp.sw_on ? p->dp.sw_steps : 0), 0, p->dp, W, B);
    hipLaunchKernelGGL(k_debug_unchord, dim3((B + 63) / 64), dim3(64), 0, 0, W, B);
    hipLaunchKernelGGL(k_refine_add, dim3(B), dim3(512), 0, 0, p->dp, W, B);
  }
  hipLaunchKernelGGL(k_residual, dim3(B), dim3(512), 0, 0, p->dp, W, B, d_out, 0);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(res_rel_out, d_out, B * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && dx_out && copy_dx_out(p, W, B, dx_out)) e = hipErrorUnknown;
  (void)hipFree(d_out);
  if (e != hipSuccess) { p->err = std::string("qtos_debug_residual: ") + hipGetErrorString(e); return -2; }
  return 0;
}

int qtos_build_flags(void) {
  int f = 0;   // (bit 0 is reserved: always 0)
#ifdef QTOS_STAMPS
  f |= 2;
#endif
#ifdef QTOS_DEV_F128
  f |= 4;
#endif
  return f;
}
int qtos_kkt_kernel(const QtosPlanner *p, char *buf, int n) {
  if (!p) return -1;
  return kkt_kernel_name(p->kkt, p->S, buf, n);
}
// Host-only: the name qtos_kkt_kernel would report for a planner created now (choose_kernel); < 0 where the analysis fails
int qtos_analyze_kernel(const QtosParams *params, char *buf, int n) {
  Analysis A;
  Kkt kind;
  if (!params || choose_kernel(*params, QtosEnv::parse(), kind, A)) return -1;
  return kkt_kernel_name(kind, A.S, buf, n);
}
/* diagnostic: the stage stream of problem b (qtos_debug_stream_len doubles) */
int qtos_debug_stream_len(const QtosPlanner *p) { return p ? (int)p->S.pack_src.size() : -1; }
int qtos_debug_read_stream(QtosPlanner *p, int b, double *out) {
  if (!p || !out || b < 0 || b >= p->max_batch) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  HIPCHK(p, hipMemcpy(out, p->wk.stream + (size_t)b * p->S.pack_src.size(), p->S.pack_src.size() * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
/* diagnostic: the vector W.rhs of problem b by position of the elimination order (n_stages x 16 doubles; S.n_unknowns counts
 * positions, dummy pivots included): after qtos_debug_residual the residual */
int qtos_debug_read_rhs(QtosPlanner *p, int b, double *out) {
  if (!p || !out || b < 0 || b >= p->max_batch) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  HIPCHK(p, hipMemcpy(out, p->wk.rhs + (size_t)b * p->S.n_unknowns, p->S.n_unknowns * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int qtos_debug_structure(const QtosPlanner *p, int *row_kind, int *var_free, int *order) {
  if (!p) return -1;
  if (row_kind) std::memcpy(row_kind, p->M.row_kind.data(), p->M.n_cons * sizeof(int));
  if (var_free)
    for (int v = 0; v < p->M.n_vars; ++v) var_free[v] = p->M.is_free(v) ? 1 : 0;
  if (order) {   // n_stages x 16 positions: the unknown eliminated there (variable, or n_vars + row), -1 = dummy pivot
    std::memcpy(order, p->S.order.data(), p->S.n_unknowns * sizeof(int));
    for (int i = p->S.n_unknowns; i < p->S.n_stages * PIV; ++i) order[i] = -1;
  }
  return 0;
}

int qtos_debug_factor(QtosPlanner *p, int b, double *panel_out, int *piv_slot_out) {
  if (!p || b < 0 || b >= p->max_batch) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  if (panel_out)
    HIPCHK(p, hipMemcpy(panel_out, p->wk.panel + (size_t)b * p->dp.panel_stride, (size_t)p->dp.panel_stride * sizeof(double), hipMemcpyDeviceToHost));
  if (panel_out) {   // rows the kernel does not store (dead slots, the stage's own pivots) are zero by definition
    const int F = p->S.front, NS = p->S.n_stages;
    for (int k = 0; k < NS; ++k)
      for (int r = 0; r < F; ++r)
        if (!((p->S.amask[(size_t)k * 8 + (r >> 5)] >> (r & 31)) & 1u))
          std::memset(panel_out + ((size_t)k * (F + 1) + 1 + r) * PIV, 0, PIV * sizeof(double));
  }
  if (piv_slot_out) std::memcpy(piv_slot_out, p->S.piv_slot.data(), p->S.piv_slot.size() * sizeof(int));
  return 0;
}

int qtos_debug_duals(QtosPlanner *p, int B, double *s, double *zl, double *zu, double *y) {
  if (!p || B < 1 || B > p->max_batch) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  HIPCHK(p, hipStreamSynchronize(p->last_stream));
  const size_t m = p->M.n_cons, NP = (size_t)p->S.n_stages * PIV;
  if (s) HIPCHK(p, hipMemcpy(s, p->wk.s, (size_t)B * m * sizeof(double), hipMemcpyDeviceToHost));
  if (zl) HIPCHK(p, hipMemcpy(zl, p->wk.zl, (size_t)B * m * sizeof(double), hipMemcpyDeviceToHost));
  if (zu) HIPCHK(p, hipMemcpy(zu, p->wk.zu, (size_t)B * m * sizeof(double), hipMemcpyDeviceToHost));
  if (y) {
    std::vector<double> sol((size_t)B * NP);
    std::vector<int> it(B);
    HIPCHK(p, hipMemcpy(sol.data(), p->wk.sol, sol.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(p, hipMemcpy(it.data(), p->wk.iters, B * sizeof(int), hipMemcpyDeviceToHost));
    std::memset(y, 0, (size_t)B * m * sizeof(double));
    // (a multiplier's id in the order is n_sol + row: behind ALL solver variables, the reduced base's coefficients included --
    //  counted from n_vars a coefficient would be read as a multiplier and the multipliers land n_coef rows too far, the last
    //  problem's behind the caller's array)
    const int n = p->M.n_sol;
    for (int b = 0; b < B; ++b)
      if (it[b] > 0)   // (a problem that took no step has no KKT solve of its own)
        for (int q = 0; q < p->S.n_unknowns; ++q)
          if (p->S.order[q] >= n) y[(size_t)b * m + (p->S.order[q] - n)] = sol[(size_t)b * NP + q];
  }
  return 0;
}

int qtos_debug_trace(QtosPlanner *p, int b, double *trace_out) {
  if (!p || b < 0 || b >= p->max_batch || !trace_out) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  int iters = 0;
  HIPCHK(p, hipMemcpy(&iters, p->wk.iters + b, sizeof(int), hipMemcpyDeviceToHost));
  const int rows = iters + 1, stride = p->M.P.max_iter + 1;
  // the caller's buffer holds max_iter + 1 rows (diagnostic builds park phase stamps past `rows`)
  HIPCHK(p, hipMemcpy(trace_out, p->wk.trace + (size_t)b * stride * 4, (size_t)stride * 4 * sizeof(double), hipMemcpyDeviceToHost));
  return rows;
}

// ---- create-time self-test of the elimination order (include/qtos_planner.h: qtos_planner_selftest) -----------------------
// The random inputs: counter-based, formed on the host (the device's log / cos / pow round differently from the host's).
//   mix(z):      z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
//   bits(i):     mix(mix(mix(mix(seed) ^ problem) ^ array) ^ i)         array: 0 dx0, 1 sig, 2 w
//   u(i):        ((bits(i) >> 11) + 0.5) * 2^-53                        in (0, 1)
//   normal(i):   sqrt(-2 log u(2 i)) * cos(2 pi u(2 i + 1))             Box-Muller, one normal per pair
static inline unsigned long long st_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static inline unsigned long long st_key(unsigned long long seed, int problem, int array) {
  return st_mix(st_mix(st_mix(seed) ^ (unsigned long long)problem) ^ (unsigned long long)array);
}
static inline double st_uniform(unsigned long long key, unsigned long long i) { return ((double)(st_mix(key ^ i) >> 11) + 0.5) * 0x1p-53; }
static inline double st_normal(unsigned long long key, unsigned long long i) {
  const double two_pi = 6.283185307179586;
  return std::sqrt(-2.0 * std::log(st_uniform(key, 2 * i))) * std::cos(two_pi * st_uniform(key, 2 * i + 1));
}
static void selftest_fill(unsigned long long seed, int b, int n, int m, double *dx0, double *sig, double *w) {
  const unsigned long long k0 = st_key(seed, b, 0), k1 = st_key(seed, b, 1), k2 = st_key(seed, b, 2);
  for (int i = 0; i < n; ++i) dx0[i] = 0.01 * st_normal(k0, i);
  for (int r = 0; r < m; ++r) {
    sig[r] = std::pow(10.0, -3.0 + 6.0 * st_uniform(k1, r));
    w[r] = st_normal(k2, r) * std::sqrt(sig[r]);
  }
}
// the two problems' start and goal: at rest at the origin in nominal stance, 0.09 m per second of horizon straight ahead
static void selftest_problem(const QtosParams &P, double *start, double *goal) {
  double T = 0.0;
  for (int k = 0; k < P.n_phases[0]; ++k) T += P.phase_dur[0][k];
  std::memset(start, 0, QTOS_START_DOUBLES * sizeof(double));
  start[2] = -P.nominal_stance[0][2];
  for (int e = 0; e < NEE; ++e) { start[6 + 3 * e] = P.nominal_stance[e][0]; start[7 + 3 * e] = P.nominal_stance[e][1]; }
  goal[0] = 0.09 * T; goal[1] = 0.0; goal[2] = start[2];
}

unsigned long long qtos_selftest_bits(unsigned long long seed, int problem, int array, unsigned long long index) {
  return st_mix(st_key(seed, problem, array) ^ index);
}
int qtos_selftest_problem(const QtosParams *params, double *start, double *goal) {
  if (!params || !start || !goal) return -1;
  selftest_problem(*params, start, goal);
  return 0;
}
int qtos_selftest_inputs(const QtosParams *params, unsigned long long seed, int b, double *dx0, double *sig, double *w) {
  if (!params || b < 0 || !dx0 || !sig || !w) return -1;
  HostModel M;   // (n_vars and n_cons do not depend on the elimination order)
  if (M.build(*params)) { fprintf(stderr, "qtos: %s\n", M.err.c_str()); return -1; }
  selftest_fill(seed, b, M.n_vars, M.n_cons, dx0, sig, w);
  return 0;
}

// nodes = towr's guess + the perturbation (a plain sum: what numpy forms from the same two arrays)
__global__ __launch_bounds__(256) void k_selftest_nodes(const double *guess, double *nodes, size_t count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) nodes[i] += guess[i];
}

// The largest |entry| of the V part of a problem's factor panels (rows 1 .. front of every stage: the rows the stage's mask
// says are stored -- the others hold whatever an earlier solve left) and the first stage that holds it.  One workgroup per
// problem, a lane per 16 bytes of a row; the waves' results meet in LDS, thread 0 stores the two numbers.  A NaN counts as inf.
__global__ __launch_bounds__(256) void k_panel_absmax(DevPlan P, DevWork W, int B, double *out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B) return;
  const int F = P.front, NS = P.n_stages;
  const double *pan = W.panel + (size_t)b * P.panel_stride;
  double mx = 0.0;
  int st = 0;
  for (int k = 0; k < NS; ++k) {
    const d2_t *V = (const d2_t *)(pan + ((size_t)k * (F + 1) + 1) * PIV);
    const unsigned *mask = P.amask + (size_t)k * 8;
    for (int i = tid; i < F * (PIV / 2); i += blockDim.x) {
      const int r = i / (PIV / 2);
      if (!((mask[r >> 5] >> (r & 31)) & 1u)) continue;
      const d2_t v = V[i];
      double a = fmax(fabs(v.x), fabs(v.y));
      if (v.x != v.x || v.y != v.y) a = INFINITY;
      if (a > mx) { mx = a; st = k; }
    }
  }
  for (int s = 32; s > 0; s >>= 1) {
    const double om = __shfl_xor(mx, s);
    const int os = __shfl_xor(st, s);
    if (om > mx || (om == mx && os < st)) { mx = om; st = os; }
  }
  __shared__ double wm[4];
  __shared__ int ws[4];
  if ((tid & 63) == 0) { wm[tid >> 6] = mx; ws[tid >> 6] = st; }
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < 4; ++j)
      if (wm[j] > mx || (wm[j] == mx && ws[j] < st)) { mx = wm[j]; st = ws[j]; }
    out[2 * b] = mx;
    out[2 * b + 1] = (double)st;
  }
}
static_assert(PIV % 2 == 0, "k_panel_absmax reads a row in pairs");

int qtos_planner_selftest(QtosPlanner *p, unsigned long long seed, double tol_residual, QtosSelftest *out) {
  if (!p || !out) return -1;
  if (p->call_open || p->busy.load()) { p->err = "qtos_planner_selftest: a call is open"; return -5; }
  const auto t_begin = std::chrono::steady_clock::now();
  std::memset(out, 0, sizeof(*out));
  const HostModel &M = p->M;
  const Symbolic &S = p->S;
  out->order_rule = M.order_rule; out->front = S.front; out->n_stages = S.n_stages;
  out->growth_limit = 1.05 / M.P.eps_dual;
  out->tol_residual = tol_residual > 0 ? tol_residual : 1e-6;
  out->residual_refined = -1.0;
  HIPCHK(p, hipSetDevice(p->device));
  HIPCHK(p, hipStreamSynchronize(p->last_stream));   // (the last call's kernels own the workspace until then)
  const int N_PROBLEMS = 2, Bc = std::min(N_PROBLEMS, p->max_batch);
  const size_t n = M.n_vars, m = M.n_cons;
  // flat ground and towr's straight-line guess whatever the handle carries: the copy of the plan the kernels get has no maps, no table
  DevPlan D = p->dp;
  D.n_maps = 0; D.height = nullptr; D.table = nullptr; D.tab_dx = D.tab_dy = nullptr; D.tab_ndx = D.tab_ndy = 0;
  std::vector<double> start((size_t)Bc * QTOS_START_DOUBLES), goal((size_t)Bc * 3), dx0(Bc * n), sig(Bc * m), w(Bc * m);
  const int N_OUT = 4;   // per problem: residual, refined residual, max |V|, its stage
  double *d_out = nullptr, h_out[2 * 4];
  HIPCHK(p, hipMalloc((void **)&d_out, (size_t)Bc * N_OUT * sizeof(double)));
  hipStream_t st = p->own_stream;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
  for (int b0 = 0; b0 < N_PROBLEMS && e == hipSuccess; b0 += Bc) {
    for (int j = 0; j < Bc; ++j) {
      selftest_problem(M.P, start.data() + (size_t)j * QTOS_START_DOUBLES, goal.data() + (size_t)j * 3);
      selftest_fill(seed, b0 + j, (int)n, (int)m, dx0.data() + j * n, sig.data() + j * m, w.data() + j * m);
    }
    DevWork W = p->wk;
    W.start = p->d_start; W.goal = p->d_goal; W.map_id = nullptr; W.warm = nullptr;
    ok(hipMemcpyAsync(p->d_start, start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ok(hipMemcpyAsync(p->d_goal, goal.data(), goal.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ok(hipMemcpyAsync(p->d_warm, dx0.data(), dx0.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ok(hipMemcpyAsync(W.sig, sig.data(), sig.size() * sizeof(double), hipMemcpyHostToDevice, st));
    ok(hipMemcpyAsync(W.w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_debug_guess, dim3(Bc), dim3(256), 0, st, D, W, Bc, p->d_nodes);
    hipLaunchKernelGGL(k_selftest_nodes, dim3((unsigned)((Bc * n + 255) / 256)), dim3(256), 0, st, p->d_nodes, p->d_warm, Bc * n);
    W.warm = p->d_warm;
    hipLaunchKernelGGL(k_debug_eval, dim3(Bc), dim3(256), p->eval_lds, st, D, W, Bc);
    hipLaunchKernelGGL(k_debug_pack, dim3(Bc), dim3(256), 0, st, D, W, Bc);
    hipLaunchKernelGGL(p->kkt_fn, dim3(Bc), dim3(p->kkt_threads), p->kkt_lds, st, D, W, Bc);
    hipLaunchKernelGGL(k_panel_absmax, dim3(Bc), dim3(256), 0, st, D, W, Bc, d_out + 2 * Bc);
    if (D.n_rec) hipLaunchKernelGGL(k_recover_dx, dim3(Bc), dim3(256), 0, st, D, W, Bc);   // (as qtos_debug_newton hands dx out)
    hipLaunchKernelGGL(k_residual, dim3(Bc), dim3(512), 0, st, D, W, Bc, d_out, p->chord_fn ? 1 : 0);   // r -> W.rhs, x remembered
    if (p->chord_fn) {   // one step of refinement, as qtos_debug_residual(refine = 1)
      hipLaunchKernelGGL(k_debug_flag_chord, dim3((Bc + 63) / 64), dim3(64), 0, st, W, Bc);
      hipLaunchKernelGGL(p->chord_fn, dim3(Bc), dim3(KTC), chord_lds_bytes(S.n_stages, D.sw_on ? D.sw_steps : 0), st, D, W, Bc);
      hipLaunchKernelGGL(k_debug_unchord, dim3((Bc + 63) / 64), dim3(64), 0, st, W, Bc);
      hipLaunchKernelGGL(k_refine_add, dim3(Bc), dim3(512), 0, st, D, W, Bc);
      hipLaunchKernelGGL(k_residual, dim3(Bc), dim3(512), 0, st, D, W, Bc, d_out + Bc, 0);
    }
    ok(hipGetLastError());
    ok(hipMemcpyAsync(h_out, d_out, (size_t)Bc * N_OUT * sizeof(double), hipMemcpyDeviceToHost, st));
    ok(hipStreamSynchronize(st));
    if (e != hipSuccess) break;
    for (int j = 0; j < Bc; ++j) {
      const double res = h_out[j], res2 = h_out[Bc + j], vmax = h_out[2 * Bc + 2 * j];
      // (a NaN is the worst result there is)
      auto worse = [](double a, double c) { return a != a || c <= a ? a : c; };
      out->residual = worse(out->residual, res);
      if (p->chord_fn) out->residual_refined = out->n_problems == 0 ? res2 : worse(out->residual_refined, res2);
      if (out->n_problems == 0 || vmax > out->max_factor) { out->max_factor = vmax; out->worst_stage = (int)h_out[2 * Bc + 2 * j + 1]; }
      out->n_problems++;
    }
  }
  (void)hipFree(d_out);
  if (e != hipSuccess) { p->err = std::string("qtos_planner_selftest: ") + hipGetErrorString(e); return -2; }
  out->passed = out->residual <= out->tol_residual && out->max_factor <= out->growth_limit;
  out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
  return 0;
}

int qtos_analyze_candidates(const QtosParams *params, int rules_mask, int *rules, int *fronts, int *stages, int n) {
  if (!params || n < 0) return -1;
  const std::vector<Candidate> c = order_candidates(*params, QtosEnv::parse(), rules_mask);
  for (int i = 0; i < (int)c.size() && i < n; ++i) {
    if (rules) rules[i] = c[i].rule;
    if (fronts) fronts[i] = c[i].front;
    if (stages) stages[i] = c[i].stages;
  }
  return (int)c.size();
}

int qtos_planner_create_checked(const QtosParams *params, int max_batch, int device, int rules_mask, double tol_residual,
                                QtosPlanner **out, QtosSelftest *tried, int max_tried, int *n_tried) {
  if (n_tried) *n_tried = 0;
  if (out) *out = nullptr;
  if (!params || !out || max_batch < 1 || max_batch >= MAX_BATCH_LIMIT || (max_tried > 0 && !tried) || max_tried < 0) return -1;
  const QtosEnv env = QtosEnv::parse();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {   // (before any analysis: nothing can be tested)
    fprintf(stderr, "qtos: no HIP device %d (found %d) -- the planner has no CPU fallback\n", device, ndev);
    return -2;
  }
  std::vector<Candidate> cand = order_candidates(*params, env, rules_mask);
  std::vector<QtosSelftest> log;
  int first_rc = 0, n_built = 0;
  for (Candidate &c : cand) {
    QtosSelftest t;
    std::memset(&t, 0, sizeof(t));
    t.order_rule = c.rule; t.residual_refined = -1.0;
    QtosPlanner *made = nullptr;
    int rc = c.ok ? create_planner(params, max_batch, device, env, c.rule, &made, c.A.get()) : -1;
    std::unique_ptr<QtosPlanner> p(made);   // (a candidate that is not handed out goes at the end of its turn)
    c.A.reset();
    if (rc == 0) {
      ++n_built;
      rc = qtos_planner_selftest(p.get(), 0, tol_residual, &t);
      if (rc) fprintf(stderr, "qtos: %s\n", p->err.c_str());
    }
    if (rc && !first_rc) first_rc = rc;
    if (rc) { t.passed = 0; t.front = 0; }
    log.push_back(t);
    if ((int)log.size() <= max_tried) tried[log.size() - 1] = t;
    if (n_tried) *n_tried = std::min((int)log.size(), max_tried);
    if (rc == 0 && t.passed) { *out = p.release(); return 0; }
  }
  if (!n_built) return first_rc ? first_rc : -1;
  fprintf(stderr, "qtos: no elimination order passed the KKT self-test:");
  for (const QtosSelftest &t : log)
    if (t.front) fprintf(stderr, " rule %d (front %d): residual %.2e (limit %.1e), max |V| %.3e (limit %.3e) in stage %d;", t.order_rule, t.front, t.residual, t.tol_residual, t.max_factor, t.growth_limit, t.worst_stage);
    else fprintf(stderr, " rule %d: not built;", t.order_rule);
  fprintf(stderr, "\n");
  return -6;
}

}  // extern "C"
