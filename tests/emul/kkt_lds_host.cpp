// kkt_lds_host.cpp -- csrc/kkt_lds.hpp under g++ (test infrastructure, compiled by tests/test_kkt_lds_cpu.py): the layouts'
// numbers, and the carves run on an array of the caller's -- every pointer comes back as its distance in bytes from the array's
// start.  Nothing is decided here but by the header.
#include "kkt_lds.hpp"

using namespace qtos;

static long long off(const void *p, const void *base) { return (const char *)p - (const char *)base; }

extern "C" {

// out = {PLD, LDS_LIMIT, SWEEP_TABLE_INTS, SW_ROUND, PIV}
void kl_constants(long long *out) {
  const long long v[5] = {PLD, (long long)LDS_LIMIT, SWEEP_TABLE_INTS, SW_ROUND, PIV};
  for (int i = 0; i < 5; ++i) out[i] = v[i];
}

// ---- k_kkt2 / k_kkt3: out = {F, FR, PSZ, NBUF, VP, LIB, DVB, DGB, UF, XS, RED, PSB, HIB, JM, PM, MIV, PB, PMB, VAR}
void kl2_layout(int F, int *out) {
  constexpr Kkt2Lds C = Kkt2Lds::of(96);   // (a compile-time constant, as the kernels read it)
  static_assert(C.PB == 1890 && C.VAR == 8470 && C.NBUF == 2 && C.VP, "Kkt2Lds::of(96)");
  const Kkt2Lds L = Kkt2Lds::of(F);
  const int v[19] = {L.F, L.FR, L.PSZ, L.NBUF, L.VP ? 1 : 0, L.LIB, L.DVB, L.DGB, L.UF, L.XS, L.RED, L.PSB, L.HIB, L.JM, L.PM, L.MIV, L.PB, L.PMB, L.VAR};
  for (int i = 0; i < 19; ++i) out[i] = v[i];
}
// out = {dbuf_doubles, sbuf_ints, hiall_ints, padded cells, end_bytes, sweep_tables, sweep_xp, sweep_base_bytes, bytes,
//        panels_bytes(3), panels_bytes(2), records_bytes, cells_bytes, fixed_bytes}
void kl2_sizes(int F, int NS, int max_srec, int max_drec, int n_cells, long long *out) {
  const Kkt2Lds L = Kkt2Lds::of(F);
  const long long v[14] = {(long long)L.dbuf_doubles(max_drec), (long long)L.sbuf_ints(max_srec), L.hiall_ints(NS), (long long)lds_cells(n_cells),
                           (long long)L.end_bytes(NS, max_srec, max_drec, n_cells), L.sweep_tables(), L.sweep_xp(NS), (long long)L.sweep_base_bytes(NS),
                           (long long)L.bytes(NS, max_srec, max_drec, n_cells), (long long)L.panels_bytes(3), (long long)L.panels_bytes(2),
                           (long long)L.records_bytes(max_srec, max_drec), (long long)L.cells_bytes(n_cells),
                           (long long)L.fixed_bytes(NS, max_srec, max_drec, n_cells)};
  for (int i = 0; i < 14; ++i) out[i] = v[i];
}
// the carve on the array lds: out = {dbuf0, sbuf0, hiall, cells (bytes from lds), dstride, sstride}
void kl2_carve(int F, int NS, int max_srec, int max_drec, double *lds, long long *out) {
  const Kkt2Lds L = Kkt2Lds::of(F);
  const Kkt2Lds::Buffers b = L.buffers(lds + L.VAR, NS, max_srec, max_drec);
  const long long v[6] = {off(b.dbuf0, lds), off(b.sbuf0, lds), off(b.hiall, lds), off(b.cells, lds), b.dstride, b.sstride};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
}

// ---- k_kkt5: out = {F, FR, PR, PSZ, MIV, L21, LIN, DVN, RSC, DGB, UF, XS, RED, PSB, PM, JM, PAN, VAR}
void kl5_layout(int F, int *out) {
  constexpr Kkt5Lds C = Kkt5Lds::of(96);
  static_assert(C.PAN == 2188 && C.VAR == 8852, "Kkt5Lds::of(96)");
  const Kkt5Lds L = Kkt5Lds::of(F);
  const int v[18] = {L.F, L.FR, L.PR, L.PSZ, L.MIV, L.L21, L.LIN, L.DVN, L.RSC, L.DGB, L.UF, L.XS, L.RED, L.PSB, L.PM, L.JM, L.PAN, L.VAR};
  for (int i = 0; i < 18; ++i) out[i] = v[i];
}
// out = {dbuf_doubles, sbuf_ints, padded cells, end_bytes, sweep_tables, sweep_xp, sweep_base_bytes, bytes}
void kl5_sizes(int F, int NS, int max_srec, int max_drec, int n_cells, long long *out) {
  const Kkt5Lds L = Kkt5Lds::of(F);
  const long long v[8] = {(long long)L.dbuf_doubles(max_drec), (long long)L.sbuf_ints(max_srec), (long long)lds_cells(n_cells),
                          (long long)L.end_bytes(max_srec, max_drec, n_cells), L.sweep_tables(), L.sweep_xp(NS), (long long)L.sweep_base_bytes(NS),
                          (long long)L.bytes(NS, max_srec, max_drec, n_cells)};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
}
// out = {dbuf, sbuf, cells (bytes from lds)}
void kl5_carve(int F, int max_srec, int max_drec, double *lds, long long *out) {
  const Kkt5Lds L = Kkt5Lds::of(F);
  const Kkt5Lds::Buffers b = L.buffers(lds + L.VAR, max_srec, max_drec);
  out[0] = off(b.dbuf, lds); out[1] = off(b.sbuf, lds); out[2] = off(b.cells, lds);
}

// ---- the sweep behind its tables and k_chord's dynamic part
// out = {the rounds (bytes from xp), sweep_ds_lds_bytes}
void kl_sweep(int NS, int sw_steps, double *xp, long long *out) {
  out[0] = off(sweep_rounds(xp, NS), xp);
  out[1] = (long long)sweep_ds_lds_bytes(NS, sw_steps);
}
// out = {xp (bytes from the tables), chord_lds_bytes}
void kl_chord(int NS, int sw_steps, int *tables, long long *out) {
  out[0] = off(chord_xp(tables, NS), tables);
  out[1] = (long long)chord_lds_bytes(NS, sw_steps);
}

}
