// call_schedule_host.cpp -- csrc/call_schedule.hpp under g++ (test infrastructure, compiled by tests/test_call_schedule_cpu.py):
// the header's functions one by one, and a handle of one lane that uses them the way qtos_plan_submit and qtos_plan_poll do, with
// the launches handed to the caller (the test's device model) instead of a stream.  Nothing is decided here but by the header.
#include "call_schedule.hpp"

#include <cstring>

using namespace qtos;

extern "C" {

// ---- words
unsigned long long cs_pack(unsigned n, unsigned nc, unsigned seq) { return pack_counts(n, nc, seq); }
int cs_read(unsigned long long word, unsigned seq, int *n, int *nc) { return read_counts(word, seq, n, nc) ? 1 : 0; }
unsigned cs_next_seq(unsigned seq) { return next_seq(seq); }
int cs_max_batch_limit() { return MAX_BATCH_LIMIT; }
int cs_sat_out_base() { return SAT_OUT_BASE; }
int cs_sat_out_code(int slot) { return sat_out_code(slot); }
int cs_sat_out_slot(int code) { return sat_out_slot(code); }
int cs_informed_kinds(int n, int nc, int slot) { return informed_kinds(n, nc, slot); }
int cs_kind_kkt() { return KIND_KKT; }
int cs_kind_chord() { return KIND_CHORD; }

// ---- layout: out = {count ints, events, call begin, call end, end of k_start, ints per count slot, sat-out int, worked int}
void cs_layout(int max_slots, int *out) {
  const SlotLayout L{max_slots};
  const int v[8] = {L.count_ints(), L.n_events(), EV_CALL_BEGIN, EV_CALL_END, L.ev_start_end(), COUNT_INTS, SAT_OUT_AT, WORKED_AT};
  std::memcpy(out, v, sizeof(v));
}
int cs_counts_at(int max_slots, int chk) { return SlotLayout{max_slots}.counts_at(chk); }
int cs_slot_event(int max_slots, int slot, int which) { return SlotLayout{max_slots}.ev(slot, (SlotEvent)which); }
int cs_events_per_slot() { return EVENTS_PER_SLOT; }

// ---- lane split: the parts into first[] and size[] (n_lanes entries at the most); returns the lanes used
int cs_split(int B, int chunk, int n_lanes, int *first, int *size) {
  const LaneSplit S(B, chunk, n_lanes);
  for (int j = 0; j < S.n_used && j < n_lanes; ++j) { first[j] = S.first(j); size[j] = S.size(j); }
  return S.n_used;
}

// ---- a handle of one lane
struct Handle {
  SlotLayout L;
  LaneProgress lane;
  LaunchPattern pattern;
  std::vector<int> counts;   // the lane's count slots: the caller stores the words k_post_counts would
  unsigned seq = 0;
  int last_iters = 1, blind_cap = 1, max_iter = 0;
};

Handle *cs_new(int max_iter, int max_slots, int has_chord, int pattern_on) {
  Handle *h = new Handle;
  h->L.max_slots = max_slots; h->max_iter = max_iter;
  h->counts.assign(h->L.count_ints(), 0);
  h->lane.ran.assign(max_slots + 1, 0);
  h->lane.kinds_mask = has_chord ? KIND_KKT | KIND_CHORD : KIND_KKT;
  h->pattern.on = pattern_on != 0;
  return h;
}
void cs_free(Handle *h) { delete h; }
int *cs_counts(Handle *h) { return h->counts.data(); }
void cs_set_speculation(Handle *h, int cap) { h->blind_cap = cap; }
void cs_set_pattern(Handle *h, int on) { h->pattern.on = on != 0; if (!on) h->pattern.clear(); }

// One launch handed out: {slot, kinds, 1 if the counts behind it are posted}.
static void hand_out(const Handle *h, int slot, int *launch, int *n) {
  launch[3 * *n] = slot; launch[3 * *n + 1] = h->lane.ran[slot]; launch[3 * *n + 2] = h->lane.reads(slot + 1) ? 1 : 0;
  ++*n;
}
// qtos_plan_submit for a call of one lane: the count slots reset, the launches queued at once.  Returns the call's sequence
// number; *start_posts: k_start's counts are posted.
unsigned cs_submit(Handle *h, int *launch, int *n_launch, int *start_posts) {
  h->seq = next_seq(h->seq);
  h->lane.begin(h->pattern.serving(1, h->blind_cap), blind_slots(h->last_iters, h->blind_cap, h->max_iter), h->L);
  std::memset(h->counts.data(), 0xff, h->counts.size() * sizeof(int));
  *start_posts = h->lane.reads(0) ? 1 : 0;
  *n_launch = 0;
  for (int it = 0; it < h->lane.spec; ++it) hand_out(h, it, launch, n_launch);
  return h->seq;
}
// qtos_plan_poll: returns 1 when the call is through (the pattern of the next call is learnt then), 0 while it waits for counts.
int cs_poll(Handle *h, int *launch, int *n_launch) {
  *n_launch = 0;
  if (!h->lane.open) return 1;   // (no call is open)
  for (int slot = 0;;) {
    const LaneProgress::Act act = h->lane.next(h->counts.data(), h->L, h->seq, &slot);
    if (act == LaneProgress::QUEUE) hand_out(h, slot, launch, n_launch);
    else if (act == LaneProgress::WAIT) return 0;
    else if (act == LaneProgress::FINISHED) break;
  }
  h->last_iters = h->lane.last_launches;
  h->pattern.update(h->lane.ran, h->lane.last_launches, h->lane.sat_out);
  return 1;
}
// out = {last_launches, n_informed, spec, enq, by_pattern, open, pattern calls, pattern misses, pattern length}; ran: max_slots + 1
// kinds; pat: the next pattern (max_slots + 1 entries at the most).
void cs_state(const Handle *h, long long *out, int *ran, int *pat) {
  const LaneProgress &c = h->lane;
  const long long v[9] = {c.last_launches, c.n_informed, c.spec, c.enq, c.by_pattern, c.open, h->pattern.calls, h->pattern.misses, (long long)h->pattern.pat.size()};
  std::memcpy(out, v, sizeof(v));
  for (size_t i = 0; i < c.ran.size(); ++i) ran[i] = c.ran[i];
  for (size_t i = 0; i < h->pattern.pat.size() && i < c.ran.size(); ++i) pat[i] = h->pattern.pat[i];
}
}
