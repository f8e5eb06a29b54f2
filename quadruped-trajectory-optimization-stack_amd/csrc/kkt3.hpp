// kkt3.hpp -- k_kkt3: the factor + solve kernel for fronts of up to 128 slots without continuation records (the default up to
// 112 slots; larger fronts and records with continuation parts stay with k_kkt2).  The stage code of kkt2.hpp on another
// schedule -- the same arithmetic: bit-identical plans.  What differs:
//
//   * The assembly of record k+2 starts in phase AB, on the waves that have no job there (their cells are not the ones the
//     tile waves read in that phase: those belong to stage k+1's columns, and a retired cell is re-issued two stages later):
//     equality entries and the first AB_R targets per thread of the gather table; the rest on every wave but the factor wave
//     at the end of phase C.  -5 % per launch on 112 slots, -6 % on 96; +4 % on 128, where seven idle waves are too few
//     (profiles/r04_experiments).
//   * No special prologue: the stage loop starts two stages early (k = -2, -1 build the panels of stages 0 and 1 through the
//     same path as every other stage).
//   * The records by LDS-DMA on waves 8 and 12 only (wave 4 assembles).
//
// The template keeps its second parameter (the kernel's name in every committed profile is k_kkt3<F, 1>): MODE 0 of rounds
// 4 - 5 -- the inequality blocks G' S G condensed on the matrix core, correct and slower -- lives in
// scratch/experiments/kkt3_mode0.hpp.
#pragma once
#include "kkt2.hpp"

namespace qtos {

// The rest of a record: equality Jacobian entries and multiplier right-hand sides are distinct cells of their own (any thread).
__device__ __forceinline__ void assemble_eq(double *A, const int *sbuf, const double *dbuf, int t0, int nth) {
  const int n_ent = sbuf[0], n_rhs = sbuf[1];
  const int *eidx = sbuf + SHDR + PIV;
  const double *eval = dbuf + PIV;
  for (int i = t0; i < n_ent; i += nth) A[eidx[i]] += eval[i];
  const int *rsl = eidx + n_ent;
  const double *rval = eval + n_ent;
  for (int i = t0; i < n_rhs; i += nth) A[rsl[i]] += rval[i];
}
// targets [t_begin, t_end) of a record's gather table (kernels.hpp assemble_stage: one thread per target, fixed summation order)
__device__ __forceinline__ void assemble_targets(double *A, const int *sbuf, const double *dbuf, int t_begin, int t_end, int t0, int nth) {
  const int n_tgt = sbuf[5];
  const int *tg = sbuf + sbuf[4];                     // n_tgt + 1 ints: (cell << 12) | first contribution
  const int *cl = tg + n_tgt + 1;                     // one self-contained int per contribution
  for (int t = t_begin + t0; t < min(t_end, n_tgt); t += nth) {
    const int tv = tg[t], c0 = tv & 4095, c1 = tg[t + 1] & 4095;
    const double a_old = A[tv >> 12];
    double acc = 0;
    for (int j = c0; j < c1; ++j) acc += gather_term(dbuf, cl[j]);
    A[tv >> 12] = a_old + acc;
  }
}
template <int F, int MODE>
__global__ __launch_bounds__(KT2) void k_kkt3(DevPlan P, DevWork W, int B) {
  static_assert(Kkt2Cfg<F>::NT <= 8 && F % 16 == 0, "k_kkt3: fronts of up to 128 slots (waves 9 .. 15 must be free in phase AB)");
  static_assert(Kkt2Layout<F>::at().NBUF == 2, "k_kkt3: the records by LDS-DMA into two buffers");
  static_assert(MODE == 1, "k_kkt3: MODE 0 left the library (scratch/experiments/kkt3_mode0.hpp)");
  const int b = blockIdx.x;
  if (b >= B || W.done[b] || W.chord[b] == 1) return;   // (a problem flagged for a chord step is k_chord's)
  extern __shared__ double lds[];
  using CF = Kkt2Cfg<F>;
  using LY = Kkt2Layout<F>;
  constexpr int NT = CF::NT, NU = CF::NU, MAXT2 = CF::MAXT, FR = CF::FR, PSZ = LY::at().PSZ;
  // targets of the gather table assembled in phase AB by the waves that idle there.  Fronts of up to 96 slots: none -- with the
  // records of round 5 (reduced swings) and six tile waves the idle waves' assembly lengthens phase AB by more than it takes off
  // phase C: -0.6 % (trot) .. -1.5 % (walk, knots200, reference_compat, exp_5, mixed) per launch without it (round 6,
  // profiles/r06_experiments/kkt96_tuning.log); the equality entries stay in phase AB.  112 and 128 slots: 64, as measured
  // in round 4.
  constexpr int AB_R = F <= 96 ? 0 : 64;
  const int tid = threadIdx.x, NS = P.n_stages, n = P.n_sol;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const Kkt2Ctx<F> cx(lds, P, W, b, wv, li, lk);
  auto r3 = [](int s) { return (s + 3) % 3; };   // ring slots of the stages -2 ..
  d4_t U[MAXT2];
#pragma unroll
  for (int i = 0; i < MAXT2; ++i) U[i] = d4_t{0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < P.n_cells; i += KT2) cx.A[i] = 0.0;
  for (int i = tid; i < 3 * PSZ + F * PLD; i += KT2) cx.PB[i] = 0.0;   // (the three panels and the blanked copy behind them)
  for (int i = tid; i < PIV * PLD; i += KT2) cx.Minv[i] = 0.0;
  for (int i = tid; i < FR; i += KT2) { cx.UF[i] = 0.0; cx.xs[i] = 0.0; }
  if (tid < 16) cx.pm[tid] = 0u;
  for (int v = tid; v < n; v += KT2) cx.dx[v] = 0.0;
  // record 0 and its header; everything else of the start-up is the stage loop itself, from k = -2
  {
    const int s0 = P.srec_off[0], s1 = P.srec_off[1], d0 = P.drec_off[0], d1 = P.drec_off[1];
    for (int i = tid; i < s1 - s0; i += KT2) cx.sbuf0[i] = P.srec[s0 + i];
    for (int i = tid; i < d1 - d0; i += KT2) cx.dbuf0[i] = cx.stream[d0 + i];
  }
  __syncthreads();
  kkt2_publish_header(cx, cx.sbuf0, cx.dbuf0, 0, 0, tid);
  __syncthreads();

  Kkt2Stamps st;
  st.start(P, W, b, tid);
  int prow_next = 0;   // pivot slot li of stage k+1
  const us4_t *ctab4 = (const us4_t *)P.ctab;
  us4_t ct_cur = {0, 0, 0, 0};
  int rc_cur = 0;      // cell of the assembled rhs of pivot li of stage k+1
  const int tid_outer = tid, lane_outer = lane;
  for (int k = -2; k < NS; ++k) {
    int tid = tid_outer, lane = lane_outer;
    asm volatile("" : "+v"(tid), "+v"(lane));
    const int li = lane & 15, lk = lane >> 4;
    const int pb = (k & 1) ? 2 : 0;
    double *Pk = cx.PB + pb * PSZ, *Yk = cx.PB + PSZ, *Xn = cx.PB + (2 - pb) * PSZ;
    const bool has_next = k + 1 >= 0 && k + 1 < NS;
    st.mark(7);
    // the records of stage k+2 (landed during the previous stage; record 0: start-up above)
    double *dbuf = cx.dbuf0 + (k & 1) * cx.dstride;
    int *sbuf = cx.sbuf0 + (k & 1) * cx.sstride;
    const us4_t ct_nxt = ctab4[((size_t)min(k + 2, NS - 1) * NT + min(wv, NT - 1)) * 64 + lane];
    const int rc_nxt = P.rtab[min(k + 2, NS - 1) * PIV + li];
    // ---- AB(k) ----------------------------------------------------------------------------------------
    const Mask256 m1 = load_mask8(cx.pm + ((k + 1) & 1) * 8, lane);   // pivot slots of stage k+1
    if (wv < NT) {
      if (k >= -1) kkt2_ab_tile(cx, k, wv, li, lk, Pk, Yk, Xn, has_next, prow_next, m1, ct_cur, k >= 0 ? P.amask[k * 8 + (wv >> 1)] : 0u, r3(k + 1));
    } else if (wv == NT) {
      if (k >= -1) kkt2_ab_rhs(cx, k, lane, li, lk, Pk, Xn, has_next, prow_next, rc_cur, k >= 0);
    }
    else if (k + 2 < NS) {
      // ---- the waves without a job in this phase assemble record k+2 into the cells.  None of the cells they touch is read
      //      or retired by the tile waves here: those belong to the columns of stage k+1, and a retired cell is handed out
      //      again two stages later (Symbolic::compact_cells).
      assemble_eq(cx.A, sbuf, dbuf, (wv - NT - 1) * 64 + lane, (15 - NT) * 64);
      assemble_targets(cx.A, sbuf, dbuf, 0, AB_R * (15 - NT) * 64, (wv - NT - 1) * 64 + lane, (15 - NT) * 64);
    }
    st.mark(0);
    lds_barrier();
    st.mark(1);
    // ---- C(k) ---------------------------------------------------------------------------------------
    st.mark(8);
    if (wv == 0) {
      __builtin_amdgcn_s_setprio(3);
      if (has_next) kkt2_factor_block(cx, Xn, prow_next, cx.psb + r3(k + 1) * PIV, cx.Lib + ((k + 1) & 1) * PIV * PLD, cx.dvb + ((k + 1) & 1) * PIV, k + 1);
      __builtin_amdgcn_s_setprio(0);
    } else if (cx.is_upd) {
      kkt2_update(cx, st, U, k, NS, lane, li, lk, Pk, Yk, k >= 0);
    }
    st.mark(2);
    {
      // the targets phase AB left: every wave but the factor wave (the waves without Schur tiles first: low item indices)
      const int apos = cx.is_upd ? (15 - NU) + cx.uw : cx.uw - NU;
      if (wv >= 1 && k + 2 < NS) assemble_targets(cx.A, sbuf, dbuf, AB_R * (15 - NT) * 64, 1 << 30, apos * 64 + lane, 15 * 64);
    }
    // LDS-DMA of the records of stage k+3 into the other buffer by waves 8 and 12 (wave 12 takes the chunks with the header
    // it publishes below)
    if ((wv == 8 || wv == 12) && k + 3 < NS) kkt2_dma_records(cx, P, k + 3, wv == 12 ? 0 : 1, 2, lane);
    if (wv == 8 || wv == 12) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (wv == 12 && k + 3 < NS) {
      // header of stage k+3 from the first chunks of the record, which this wave has just waited for (the slots of the LDS
      // rings have no reader left in this phase: stage k's pivot slots / diagonals, stage k+1's slot map and mask)
      const int hs = k + 3;
      if (lane < 8) cx.pm[(hs & 1) * 8 + lane] = 0u;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      kkt2_publish_header(cx, cx.sbuf0 + (hs & 1) * cx.sstride, cx.dbuf0 + (hs & 1) * cx.dstride, hs, r3(hs), lane);
    }
    st.mark(3);
    lds_barrier();
    st.mark(4);
    if (k + 2 < NS) prow_next = cx.psb[r3(k + 2) * PIV + li];
    ct_cur = ct_nxt;
    rc_cur = rc_nxt;
  }
  __syncthreads();  // drains the factor-panel stores: they are read back below
  st.mark(7);
  kkt2_backward(cx, P, W, b, tid, wv, lane);
  st.finish();
}

}  // namespace qtos
