// call_schedule.hpp -- the launch schedule of one plan call (qtos_plan_submit / qtos_plan_poll), stated once:
//   the count word     what k_post_counts stores behind a launch slot and the host spins on, and the sat-out code next to it
//   the slot layout    where a lane's count slots and HIP events sit for a given max_slots
//   the kinds          which solve kernels a launch slot runs (bit 0 the factorising kernel, bit 1 k_chord)
//   the lane split     how a call larger than the GPU is cut into lanes
//   the lane progress  what a lane does with the counts that have arrived: wait, finish, queue the next slot, step on
//   the launch pattern what the next call of the handle queues without a look at the counts
// Plain integer C++, no HIP types: qtos_planner.hip compiles it under hipcc (QTOS_HD: what the kernels use too), and
// tests/test_call_schedule_cpu.py under g++, where it drives simulated calls against a restatement.
#pragma once
#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define QTOS_HD __host__ __device__
#else
#define QTOS_HD
#endif

namespace qtos {

// ---- the count word: bits 0 .. 23 unfinished problems, 24 .. 47 of those flagged for a chord step, 48 .. 63 the sequence number
// of the call that queued the launch.  A slot is reset to all ones: no call carries the number 0xffff (nor 0), so the reset word
// and the late store of an earlier call's blind launch both read as "no counts of this call yet".
constexpr int COUNT_BITS = 24, SEQ_SHIFT = 2 * COUNT_BITS;
constexpr unsigned COUNT_MASK = (1u << COUNT_BITS) - 1, SEQ_MASK = 0xffffu;
constexpr int MAX_BATCH_LIMIT = 1 << COUNT_BITS;   // qtos_planner_create: max_batch below it, so that a count fits its bits

QTOS_HD inline unsigned long long pack_counts(unsigned n, unsigned nc, unsigned seq) {
  return (unsigned long long)(n & COUNT_MASK) | ((unsigned long long)(nc & COUNT_MASK) << COUNT_BITS) | ((unsigned long long)(seq & SEQ_MASK) << SEQ_SHIFT);
}
// The counts of call `seq` in the word, or false: nothing of that call yet.
inline bool read_counts(unsigned long long word, unsigned seq, int *n, int *nc) {
  *n = (int)(word & COUNT_MASK); *nc = (int)((word >> COUNT_BITS) & COUNT_MASK);
  return (unsigned)(word >> SEQ_SHIFT) == seq;
}
// 1 .. 0xfffe round and round.  (A stale word is taken for this call's only if a blind launch of the call 65 534 submits earlier
// were still to store: a call is submitted after the previous one was collected, and queues at most max_iter blind launches.)
inline unsigned next_seq(unsigned seq) { return seq >= SEQ_MASK - 1 ? 1u : seq + 1u; }

// A count slot is four ints: the count word in the first two, then the code of the EARLIEST launch slot a problem sat out
// (k_step: atomicMax keeps the largest code; 0 = nobody) and the launch slots in which some problem took a step.
constexpr int COUNT_INTS = 4, SAT_OUT_AT = 2, WORKED_AT = 3;
constexpr int SAT_OUT_BASE = 1 << 20;              // qtos_planner_create: max_slots below it, so that every slot's code is positive
QTOS_HD inline int sat_out_code(int slot) { return SAT_OUT_BASE - slot; }
inline int sat_out_slot(int code) { return code > 0 ? SAT_OUT_BASE - code : -1; }   // -1: nobody sat out

// ---- the kinds of a launch slot, and the rule of an informed launch: n unfinished problems of which nc wait for a chord step
// in front of slot `slot` (no chord step in front of the first: nothing is factorised yet)
constexpr int KIND_KKT = 1, KIND_CHORD = 2;
inline int informed_kinds(int n, int nc, int slot) { return (n - nc > 0 ? KIND_KKT : 0) | (nc > 0 && slot >= 1 ? KIND_CHORD : 0); }

// ---- where things sit for a call of at most max_slots launch slots
enum SlotEvent { KKT_BEGIN, KKT_END, CHORD_BEGIN, CHORD_END, SLOT_END, EVENTS_PER_SLOT };
constexpr int EV_CALL_BEGIN = 0, EV_CALL_END = 1;   // (a lane's first kernel; the end of the call: lane 0's)
struct SlotLayout {
  int max_slots = 0;   // launch slots a call may use (iterations + launches a problem sat out)
  // ints into a lane's count slots: the counts in front of slot chk -- behind slot chk - 1, or behind k_start (the last slot)
  int counts_at(int chk) const { return COUNT_INTS * (chk == 0 ? max_slots : chk - 1); }
  int count_ints() const { return COUNT_INTS * (max_slots + 1); }
  int ev(int slot, SlotEvent e) const { return 2 + EVENTS_PER_SLOT * slot + e; }
  int ev_start_end() const { return ev(max_slots, KKT_BEGIN); }   // behind k_start and its counts
  int n_events() const { return ev_start_end() + 1; }
};

// ---- the lane split: one lane up to `chunk` problems (the GPU's compute units), then at most n_lanes equal parts of
// per = ceil(B / lanes) problems, of which ceil(B / per) are used: every part is non-empty
struct LaneSplit {
  int B, per, n_used;
  LaneSplit(int B, int chunk, int n_lanes) : B(B) {
    const int n = B <= chunk ? 1 : std::min(n_lanes, (B + chunk - 1) / chunk);
    per = (B + n - 1) / n;
    n_used = (B + per - 1) / per;
  }
  int first(int j) const { return j * per; }
  int size(int j) const { return std::min(per, B - j * per); }
};

// ---- the launch pattern of a handle: the kinds every launch slot of its last two calls ran, as far as the two agree
struct LaunchPattern {
  bool on = true;                    // qtos_set_pattern_speculation
  std::vector<char> pat, obs_prev;   // the prefix the next call queues at once; the kinds the last call's slots ran
  long long calls = 0, misses = 0;   // calls that followed a pattern; of those, calls in which a problem sat a slot out
  void clear() { pat.clear(); obs_prev.clear(); }
  int prefix(int max_slots) const { return std::min((int)pat.size(), max_slots); }
  // The pattern serves calls of one lane (a call cut into lanes keeps the informed loop per lane) without blind iterations:
  // itself, counted, for a call that follows it, or null.
  const LaunchPattern *serving(int n_lanes_used, int blind_cap) {
    if (!on || n_lanes_used != 1 || pat.empty() || blind_cap > 1) return nullptr;
    calls++;
    return this;
  }
  // Behind a call of one lane: `ran` the kinds of its slots, `launches` the slots with work, `code` the sat-out code.  A problem
  // that sat a slot out cuts the observation in front of that slot (what the slots behind it ran was the pattern's choice, not
  // the batch's).  The next pattern: the observation as far as it agrees with the last one (nothing observed yet: all of it).
  void update(const std::vector<char> &ran, int launches, int code) {
    if (code > 0) { launches = std::min(launches, sat_out_slot(code)); misses++; }
    std::vector<char> obs(ran.begin(), ran.begin() + std::max(launches, 0));
    size_t k = 0;
    if (obs_prev.empty()) k = obs.size();
    else while (k < obs.size() && k < obs_prev.size() && obs[k] == obs_prev[k]) ++k;
    pat.assign(obs.begin(), obs.begin() + k);
    obs_prev.swap(obs);
  }
};

// Blind iterations of a call (qtos_set_speculation: cap, 1 = the first iteration only): as many as the handle's last call took.
inline int blind_slots(int last_iters, int cap, int max_iter) { return std::max(0, std::min(std::min(std::max(1, last_iters), cap), max_iter)); }

// ---- one lane's progress through its call.  Slots 0 .. spec - 1 are queued at submit time: the pattern's prefix, of which only
// the last posts its counts, or blind ones (the first the factorising kernel, the others both kernels), which all do, as does
// k_start then.  From there on next() says what the counts that have arrived allow.
struct LaneProgress {
  int spec = 0, enq = 0, chk = 0;   // slots queued at submit time / queued in all / whose preceding counts have been read
  int n_informed = 0;               // launches of the call that waited for the host to read the counts
  bool by_pattern = false, open = false;   // open: from begin() until next() has said FINISHED
  int kinds_mask = KIND_KKT | KIND_CHORD;   // the solve kernels the handle has (chord steps off: KIND_KKT)
  std::vector<char> ran;            // per slot of the last call: the kinds launched, as far as they had work
  int last_launches = 0, sat_out = 0;   // of the last call: slots with work, the sat-out code behind them
  enum Act { WAIT, FINISHED, QUEUE, STEP };

  void begin(const LaunchPattern *pattern, int blind, const SlotLayout &L) {   // pattern: null for a call that does not follow it
    by_pattern = pattern != nullptr; open = true;
    spec = by_pattern ? pattern->prefix(L.max_slots) : std::min(blind, L.max_slots);
    enq = spec; chk = by_pattern ? spec : 0; n_informed = 0;   // (by pattern: the first counts read are those behind slot spec - 1)
    for (int it = 0; it < spec; ++it) ran[it] = (char)((by_pattern ? pattern->pat[it] : it >= 1 ? KIND_KKT | KIND_CHORD : KIND_KKT) & kinds_mask);
  }
  // The host reads the counts in front of slot chk (those behind slot chk - 1 or k_start, which posts them then).
  bool reads(int chk) const { return !by_pattern || chk >= spec; }
  // counts: the lane's count slots.  QUEUE: launch *slot with ran[*slot], then ask again; STEP: ask again.
  Act next(const int *counts, const SlotLayout &L, unsigned seq, int *slot) {
    const int *h = counts + L.counts_at(chk);
    int n, nc;
    if (!read_counts(__atomic_load_n((const unsigned long long *)h, __ATOMIC_ACQUIRE), seq, &n, &nc)) return WAIT;
    if (n <= 0 || chk >= L.max_slots) {
      // finished in front of slot chk.  A call that followed the pattern learns here how many of its slots had work; the others
      // read every slot's counts and stop at the first without work.  Launches queued behind the end ran nothing.
      last_launches = by_pattern ? std::max(0, std::min(h[WORKED_AT], chk)) : chk;
      sat_out = h[SAT_OUT_AT];
      std::fill(ran.begin() + last_launches, ran.begin() + enq, 0);   // (last_launches <= chk <= enq)
      open = false;
      return FINISHED;
    }
    const int kinds = informed_kinds(n, nc, chk) & kinds_mask;
    if (chk < spec && !by_pattern) ran[chk] = (char)kinds;   // a blind iteration that did run: which of its kernels had work
    *slot = chk++;
    if (*slot < enq) return STEP;
    ran[*slot] = (char)kinds;
    enq++; n_informed++;
    return QUEUE;
  }
};

}  // namespace qtos
