// kkt_lds.hpp -- where everything sits in the LDS of the factor + solve kernels (k_kkt2 / k_kkt3: Kkt2Lds, k_kkt5: Kkt5Lds), of
// k_chord and of the backward sweep, and how many bytes that takes: the one statement the kernels carve their LDS by and the
// host sizes their allocation by.  Offsets in doubles from the start of the dynamic LDS.  A layout is a constexpr value,
// Kkt2Lds::of(F): the kernels read it as compile-time constants (Kkt2Layout<F>::at()), the host at run time.  Plain C++: the
// kernels compile it under hipcc, tests/test_kkt_lds_cpu.py under g++, where the carve is run on a host array.
//
//   k_kkt2 / k_kkt3   [LIB .. MIV: fixed][PB: 3 panels][PMB: blanked copy, VP only][VAR: buffers()]    forward pass
//                     [LIB .. MIV: fixed][PB: sweep tables][xp][rounds]                                backward sweep
//   k_kkt5            [MIV .. JM: fixed][PAN: 4 panels][VAR: buffers()]  /  [fixed][PAN: sweep tables][xp][rounds]
//   k_chord           (static arrays, then dynamic:)  [sweep tables][xp][rounds]
#pragma once
#include <cstddef>

#include "symbolic.hpp"

#if defined(__HIPCC__)
#define QTOS_HD __host__ __device__
#else
#define QTOS_HD
#endif

namespace qtos {

constexpr int PLD = PIV + 1;                            // leading dimension of the 16-column LDS panels
constexpr size_t LDS_LIMIT = 160 * 1024 - 256;          // LDS one workgroup of the factor + solve kernels may claim
constexpr int SWEEP_TABLE_INTS = 12;                    // per stage: Symbolic::nxt_pack (4 ints), then Symbolic::amask2 (8)
constexpr int SW_ROUND = 16;                            // rows of a round of the sweep's helper waves

// ---- the backward sweep behind its tables: xp, the solution by position (NS x 16 doubles), then the rounds' rows (the first
//      four ints of a SwTask each) ------------------------------------------------------------------------------------------
QTOS_HD inline double *sweep_rounds(double *xp, int NS) { return xp + NS * PIV; }   // (16-byte aligned where xp is)
QTOS_HD inline size_t sweep_ds_lds_bytes(int NS, int sw_steps) {
  return sw_steps > 0 ? 16 + (size_t)NS * PIV * sizeof(double) + (size_t)sw_steps * SW_ROUND * 16 : 0;
}
// k_chord's dynamic LDS: the sweep tables, then xp
QTOS_HD inline double *chord_xp(int *tables, int NS) { return (double *)(tables + ((NS * SWEEP_TABLE_INTS + 3) & ~3)); }
inline size_t chord_lds_bytes(int NS, int sw_steps) { return sizeof(int) * (size_t)NS * SWEEP_TABLE_INTS + sweep_ds_lds_bytes(NS, sw_steps); }

// a record buffer filled by LDS-DMA (1 KB per wave instruction): whole KB
QTOS_HD constexpr size_t lds_dma_doubles(int n) { return (((size_t)n * 8 + 1023) & ~(size_t)1023) / 8; }
QTOS_HD constexpr size_t lds_dma_ints(int n) { return (((size_t)n * 4 + 1023) & ~(size_t)1023) / 4; }
QTOS_HD constexpr size_t lds_cells(int n_cells) { return ((size_t)n_cells + 1) & ~(size_t)1; }   // padded to 16 bytes

// ---- k_kkt2 / k_kkt3 ------------------------------------------------------------------------------------------------------
struct Kkt2Lds {
  int F, FR, PSZ;    // slots of the front; by-slot arrays padded to whole waves; a panel of (F + 1) x PLD
  int NBUF;          // record buffers of each kind: two, filled by LDS-DMA (record s in buffer s & 1), or one, filled through prefetch registers
  bool VP;           // update as  U -= V P^T  with operand B in a fourth panel (PMB)
  int LIB, DVB, DGB, UF, XS, RED, PSB, HIB, JM, PM, MIV, PB, PMB, VAR;
  struct Buffers {   // behind VAR: [dbuf 0][dbuf 1][sbuf 0][sbuf 1][hiall][cells]
    double *dbuf0;
    int *sbuf0, *hiall;
    double *cells;
    int dstride, sstride;
  };

  QTOS_HD static constexpr Kkt2Lds of(int F) {
    Kkt2Lds L{};
    L.F = F;
    L.FR = (F + 63) & ~63;
    L.PSZ = (F + 1) * PLD;
    L.VP = F <= 128;                          // (larger fronts have no room for the fourth panel nor for a second record buffer)
    L.NBUF = L.VP ? 2 : 1;
    L.LIB = 0;                                // 2 x 16 x PLD   L^-1 (current / next)
    L.DVB = L.LIB + 2 * PIV * PLD;            // 2 x 16         1 / d
    L.DGB = L.DVB + 2 * PIV;                  // 3 x 16         pivot diagonals (ring)
    L.UF = L.DGB + 3 * PIV;                   // FR             accumulated rhs updates
    L.XS = L.UF + L.FR;                       // FR             solution by slot (backward)
    L.RED = L.XS + L.FR;                      // 2 x 16 x 16 partial sums + 64 dummy slots
    L.PSB = L.RED + 2 * 16 * PIV + 64;        // 3 x 16 ints    pivot slots (ring)
    L.HIB = L.PSB + 3 * PIV / 2;              // 4 ints
    L.JM = L.HIB + 2;                         // 2 x FR ints    slot -> pivot index
    L.PM = L.JM + L.FR;                       // 2 x 8 ints     pivot-slot bit masks
    L.MIV = L.PM + 8;                         // 16 x PLD       (L D L^T)^-1 of the current pivot block
    L.PB = L.MIV + PIV * PLD;                 // 3 panels of (F+1) x PLD: P_k / P_k+1 alternate in 0 and 2, 1 = operand A of the update
    L.PMB = L.PB + 3 * L.PSZ;                 // F x PLD: rows of P_k with those of the next pivots blanked
    L.VAR = (L.PMB + (L.VP ? F * PLD : 0) + 1) & ~1;   // dbuf, then (ints) sbuf, hiall, then the cells
    return L;
  }
  QTOS_HD constexpr size_t dbuf_doubles(int max_drec) const { return NBUF == 2 ? lds_dma_doubles(max_drec) : (((size_t)max_drec + 1) & ~(size_t)1); }
  QTOS_HD constexpr size_t sbuf_ints(int max_srec) const { return NBUF == 2 ? lds_dma_ints(max_srec) : (((size_t)max_srec + 3) & ~(size_t)3); }
  QTOS_HD constexpr int hiall_ints(int NS) const { return (NS + 4) & ~3; }   // a stage's rounded slot count, one entry to spare
  // var = lds + VAR
  QTOS_HD Buffers buffers(double *var, int NS, int max_srec, int max_drec) const {
    Buffers b;
    b.dstride = (int)dbuf_doubles(max_drec);
    b.sstride = (int)sbuf_ints(max_srec);
    b.dbuf0 = var;
    b.sbuf0 = (int *)(b.dbuf0 + NBUF * b.dstride);
    b.hiall = b.sbuf0 + NBUF * b.sstride;
    b.cells = (double *)(b.hiall + hiall_ints(NS));
    return b;
  }
  // where the cells behind that chain end
  constexpr size_t end_bytes(int NS, int max_srec, int max_drec, int n_cells) const {
    return (VAR + NBUF * dbuf_doubles(max_drec) + lds_cells(n_cells)) * sizeof(double) + (NBUF * sbuf_ints(max_srec) + hiall_ints(NS)) * sizeof(int);
  }
  // the backward sweep: its tables where the panels were, xp behind them
  QTOS_HD constexpr int sweep_tables() const { return PB; }
  QTOS_HD constexpr int sweep_xp(int NS) const { return (PB + NS * (SWEEP_TABLE_INTS / 2) + 1) & ~1; }
  constexpr size_t sweep_base_bytes(int NS) const { return (size_t)sweep_xp(NS) * sizeof(double); }   // in front of sweep_ds_lds_bytes
  constexpr size_t bytes(int NS, int max_srec, int max_drec, int n_cells) const {
    const size_t fwd = end_bytes(NS, max_srec, max_drec, n_cells), bwd = sweep_base_bytes(NS);
    return fwd > bwd ? fwd : bwd;
  }
  // The parts qtos_analyze_two_ended reports, counted as the layout of fronts up to 128 slots has them whatever F is: n_pan
  // panels and the blanked copy, two record buffers of each kind, the cells; the fixed part is what bytes() holds besides
  // (on a larger front, which has neither the copy nor the second buffers, the three exceed bytes() and it reads 0).
  constexpr size_t panels_bytes(int n_pan = 3) const { return (size_t)(n_pan * PSZ + F * PLD) * sizeof(double); }
  constexpr size_t records_bytes(int max_srec, int max_drec) const { return 2 * (dbuf_doubles(max_drec) * sizeof(double) + sbuf_ints(max_srec) * sizeof(int)); }
  static constexpr size_t cells_bytes(int n_cells) { return lds_cells(n_cells) * sizeof(double); }
  constexpr size_t fixed_bytes(int NS, int max_srec, int max_drec, int n_cells) const {
    const size_t total = bytes(NS, max_srec, max_drec, n_cells), parts = panels_bytes() + records_bytes(max_srec, max_drec) + cells_bytes(n_cells);
    return total > parts ? total - parts : 0;
  }
};

// ---- k_kkt5 ---------------------------------------------------------------------------------------------------------------
struct Kkt5Lds {
  int F, FR, PR, PSZ;   // slots; by-slot arrays padded to whole waves; rows of a panel: the slots, the right-hand side, a row of zeros; a panel
  int MIV, L21, LIN, DVN, RSC, DGB, UF, XS, RED, PSB, PM, JM, PAN, VAR;
  struct Buffers {      // behind VAR: [dbuf][sbuf][cells], one record buffer of each kind, filled by LDS-DMA
    double *dbuf;
    int *sbuf;
    double *cells;
  };

  QTOS_HD static constexpr Kkt5Lds of(int F) {
    Kkt5Lds L{};
    L.F = F;
    L.FR = (F + 63) & ~63;
    L.PR = F + 2;
    L.PSZ = L.PR * PLD;
    L.MIV = 0;                                // 2 x 16 x PLD   A11^-1, S22^-1 of the pair being eliminated
    L.L21 = L.MIV + 2 * PIV * PLD;            // 16 x PLD       L21 = A21 A11^-1, row major
    L.LIN = L.L21 + PIV * PLD;                // 16 x PLD       scratch of the factor wave (L^-1; S22)
    L.DVN = L.LIN + PIV * PLD;                // 16             1 / d of the block being factored
    L.RSC = L.DVN + PIV;                      // 4 x 16         scratch of the right-hand-side wave
    L.DGB = L.RSC + 4 * PIV;                  // 3 x 32         pivot diagonals (ring by pair % 3)
    L.UF = L.DGB + 3 * 2 * PIV;               // FR             accumulated right-hand-side updates by slot
    L.XS = L.UF + L.FR;                       // FR             solution by slot (backward sweep)
    L.RED = L.XS + L.FR;                      // 2 x 16 x 16 partial sums of the sweep + 64 dummy slots
    L.PSB = L.RED + 2 * 16 * PIV + 64;        // 3 x 32 ints    pivot slots (ring)
    L.PM = L.PSB + 3 * 2 * PIV / 2;           // 3 x 8 words    pivot-slot bit masks (ring)
    L.JM = L.PM + 3 * 8 / 2;                  // FR ushorts     slot -> column offset of its pivot in the pair's two panels
    L.PAN = (L.JM + L.FR / 4 + 1) & ~1;       // 4 panels of PR x PLD: pair q in panels 2 (q & 1), 2 (q & 1) + 1
    L.VAR = (L.PAN + 4 * L.PSZ + 1) & ~1;     // dbuf, then (ints) sbuf, then the cells
    return L;
  }
  QTOS_HD static constexpr size_t dbuf_doubles(int max_drec) { return lds_dma_doubles(max_drec); }
  QTOS_HD static constexpr size_t sbuf_ints(int max_srec) { return lds_dma_ints(max_srec); }
  // var = lds + VAR
  QTOS_HD Buffers buffers(double *var, int max_srec, int max_drec) const {
    const int dstride = (int)dbuf_doubles(max_drec), sstride = (int)sbuf_ints(max_srec);
    Buffers b;
    b.dbuf = var;
    b.sbuf = (int *)(b.dbuf + dstride);
    b.cells = (double *)(b.sbuf + sstride);
    return b;
  }
  constexpr size_t end_bytes(int max_srec, int max_drec, int n_cells) const {
    return (VAR + dbuf_doubles(max_drec) + lds_cells(n_cells)) * sizeof(double) + sbuf_ints(max_srec) * sizeof(int);
  }
  QTOS_HD constexpr int sweep_tables() const { return PAN; }
  QTOS_HD constexpr int sweep_xp(int NS) const { return (PAN + NS * (SWEEP_TABLE_INTS / 2) + 1) & ~1; }
  constexpr size_t sweep_base_bytes(int NS) const { return (size_t)sweep_xp(NS) * sizeof(double); }
  constexpr size_t bytes(int NS, int max_srec, int max_drec, int n_cells) const {
    const size_t fwd = end_bytes(max_srec, max_drec, n_cells), bwd = sweep_base_bytes(NS);
    return fwd > bwd ? fwd : bwd;
  }
};

}  // namespace qtos
