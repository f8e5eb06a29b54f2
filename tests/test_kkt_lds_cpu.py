"""csrc/kkt_lds.hpp, the LDS layout of the factor + solve kernels, of k_chord and of the backward sweep, held on the host (no GPU).

The header is plain C++; tests/emul/kkt_lds_host.cpp (test infrastructure, compiled here with g++) returns its numbers and runs its
carves on an array of this test's.  Two things are asserted over every compiled front and a grid of stage counts, record sizes and
cell counts:

  the layout is what it was   the offsets are the prefix sums of a table of (region, doubles) per kernel, restated here, and hit
                              the values the kernels had before the header existed; the byte counts equal the closed forms the
                              host computed them by before, written out below
  the carve is sound          every region the kernel's pointer chain yields lies inside bytes(), in order and disjoint, aligned
                              as its users need; the sweep's tables start behind what the sweep still reads, and the sweep's and
                              k_chord's xp and rounds end inside their allocations
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "quadruped-trajectory-optimization-stack_amd", "csrc")
SRC = os.path.join(HERE, "emul", "kkt_lds_host.cpp")
OUT = os.path.join(HERE, "emul", "_build", "libkkt_lds_host.so")

PIV, PLD = 16, 17
FRONTS2 = list(range(16, 209, 16))          # k_kkt2 / k_kkt3 / k_chord instantiations
FRONTS5 = [96, 112, 128, 144]               # k_kkt5
NS_GRID = [1, 2, 7, 100, 113, 231]
SREC_GRID = [0, 1, 255, 256, 257, 3000, 6144]
DREC_GRID = [0, 1, 127, 128, 129, 2048]
CELL_GRID = [0, 1, 2, 999, 3000]
STEP_GRID = [0, 1, 7, 231, 400]             # rounds of the sweep's helper waves
GRID = list(itertools.product(NS_GRID, SREC_GRID, DREC_GRID, CELL_GRID))

# the layouts before the header, in doubles: (PB, VAR) of Kkt2Layout<F>, (PAN, VAR) of Kkt5Layout<F>
ANCHORS2 = {16: (1698, 2838), 32: (1698, 3926), 48: (1698, 5014), 64: (1698, 6102), 80: (1890, 7382), 96: (1890, 8470), 112: (1890, 9558),
            128: (1890, 10646), 144: (2082, 9478), 160: (2082, 10294), 176: (2082, 11110), 192: (2082, 11926), 208: (2274, 12934)}
ANCHORS5 = {96: (2188, 8852), 112: (2188, 9940), 128: (2188, 11028), 144: (2332, 12260)}


def up(x, m):
    return (x + m - 1) // m * m


@pytest.fixture(scope="module")
def lib():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "kkt_lds.hpp"), os.path.join(CSRC, "symbolic.hpp")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, SRC, "-o", OUT])
    lib = C.CDLL(OUT)
    for f in (lib.kl_constants, lib.kl2_layout, lib.kl2_sizes, lib.kl2_carve, lib.kl5_layout, lib.kl5_sizes, lib.kl5_carve, lib.kl_sweep, lib.kl_chord):
        f.restype = None
    return lib


@pytest.fixture(scope="module")
def arena():
    """The host array the carves run on: 16-byte aligned, larger than any bytes() of the grid."""
    raw = np.zeros(1 << 19, dtype=np.uint8)
    a = raw[(-raw.ctypes.data) % 16:]
    assert a.ctypes.data % 16 == 0
    return a


def ints(n):
    return (C.c_int * n)()


def longs(n):
    return (C.c_longlong * n)()


# ---------------------------------------------------------------- the header's answers
L2_NAMES = ["F", "FR", "PSZ", "NBUF", "VP", "LIB", "DVB", "DGB", "UF", "XS", "RED", "PSB", "HIB", "JM", "PM", "MIV", "PB", "PMB", "VAR"]
S2_NAMES = ["dbuf_doubles", "sbuf_ints", "hiall_ints", "cells", "end_bytes", "sweep_tables", "sweep_xp", "sweep_base_bytes", "bytes",
            "panels3", "panels2", "records", "cells_bytes", "fixed"]
L5_NAMES = ["F", "FR", "PR", "PSZ", "MIV", "L21", "LIN", "DVN", "RSC", "DGB", "UF", "XS", "RED", "PSB", "PM", "JM", "PAN", "VAR"]
S5_NAMES = ["dbuf_doubles", "sbuf_ints", "cells", "end_bytes", "sweep_tables", "sweep_xp", "sweep_base_bytes", "bytes"]


def layout2(lib, F):
    o = ints(len(L2_NAMES))
    lib.kl2_layout(F, o)
    return dict(zip(L2_NAMES, o))


def sizes2(lib, F, NS, ms, md, nc):
    o = longs(len(S2_NAMES))
    lib.kl2_sizes(F, NS, ms, md, nc, o)
    return dict(zip(S2_NAMES, o))


def layout5(lib, F):
    o = ints(len(L5_NAMES))
    lib.kl5_layout(F, o)
    return dict(zip(L5_NAMES, o))


def sizes5(lib, F, NS, ms, md, nc):
    o = longs(len(S5_NAMES))
    lib.kl5_sizes(F, NS, ms, md, nc, o)
    return dict(zip(S5_NAMES, o))


# ---------------------------------------------------------------- the restatement: regions in doubles, in order
def regions2(F):
    FR = up(F, 64)
    return [("LIB", 2 * 16 * PLD), ("DVB", 2 * 16), ("DGB", 3 * 16), ("UF", FR), ("XS", FR), ("RED", 2 * 16 * 16 + 64), ("PSB", 3 * 16 // 2),
            ("HIB", 4 // 2), ("JM", 2 * FR // 2), ("PM", 2 * 8 // 2), ("MIV", 16 * PLD), ("PB", 3 * (F + 1) * PLD),
            ("PMB", F * PLD if F <= 128 else 0)]


def regions5(F):
    FR = up(F, 64)
    return [("MIV", 2 * 16 * PLD), ("L21", 16 * PLD), ("LIN", 16 * PLD), ("DVN", 16), ("RSC", 4 * 16), ("DGB", 3 * 32), ("UF", FR), ("XS", FR),
            ("RED", 2 * 16 * 16 + 64), ("PSB", 3 * 32 // 2), ("PM", 3 * 8 // 2), ("JM", FR // 4)]


def prefix(regions):
    at, o = {}, 0
    for name, n in regions:
        at[name] = o
        o += n
    return at, o


# ---------------------------------------------------------------- the host's closed forms before the header
def old_dma(n, unit):
    return up(n * unit, 1024) // unit


def old_kkt2_fixed(F):
    FR = up(F, 64)
    return 2 * PIV * PLD + 2 * PIV + 3 * PIV + 2 * FR + 2 * 16 * PIV + 64 + 3 * PIV // 2 + 2 + FR + 8 + PIV * PLD


def old_kkt2_dbuf(F, md):
    return old_dma(md, 8) if F <= 128 else up(md, 2)


def old_kkt2_sbuf(F, ms):
    return old_dma(ms, 4) if F <= 128 else up(ms, 4)


def old_kkt2_sweep_base_bytes(F, NS):
    return old_kkt2_fixed(F) * 8 + NS * 12 * 4


def old_kkt2_lds_bytes(F, NS, ms, md, nc):
    o = up(old_kkt2_fixed(F) + 3 * (F + 1) * PLD + (F * PLD if F <= 128 else 0), 2)
    nbuf = 2 if F <= 128 else 1
    o += nbuf * old_kkt2_dbuf(F, md)
    oi = 2 * o + nbuf * old_kkt2_sbuf(F, ms) + up(NS + 1, 4)
    oi += 2 * up(nc, 2)
    return max(oi * 4, old_kkt2_sweep_base_bytes(F, NS))


def old_kkt5_fixed(F):
    FR = up(F, 64)
    o = 2 * PIV * PLD + PIV * PLD + PIV * PLD + PIV + 4 * PIV + 3 * 2 * PIV + 2 * FR + 2 * 16 * PIV + 64 + 3 * 2 * PIV // 2 + 3 * 8 // 2
    return up(o + FR // 4, 2)


def old_kkt5_sweep_base_bytes(F, NS):
    return old_kkt5_fixed(F) * 8 + NS * 12 * 4


def old_kkt5_lds_bytes(F, NS, ms, md, nc):
    o = up(old_kkt5_fixed(F) + 4 * (F + 2) * PLD, 2) + old_dma(md, 8)
    oi = 2 * o + old_dma(ms, 4) + 2 * up(nc, 2)
    return max(oi * 4, old_kkt5_sweep_base_bytes(F, NS))


def old_sweep_ds_lds_bytes(NS, steps):
    return 16 + NS * PIV * 8 + steps * 16 * 16 if steps > 0 else 0


def old_chord_lds_bytes(NS, steps):
    return 4 * NS * 12 + old_sweep_ds_lds_bytes(NS, steps)


def old_two_ended_parts(F, NS, ms, md, nc):
    """panels (3), panels (2), record buffers, cells, fixed part as qtos_analyze_two_ended computed them"""
    def panel_b(n_pan):
        return ((F + 1) * PLD * n_pan + F * PLD) * 8
    rec = 2 * (old_kkt2_dbuf(F, md) * 8 + old_kkt2_sbuf(F, ms) * 4)
    cells = up(nc, 2) * 8
    total = old_kkt2_lds_bytes(F, NS, ms, md, nc)
    return panel_b(3), panel_b(2), rec, cells, max(total - panel_b(3) - rec - cells, 0)


# ---------------------------------------------------------------- the layout is what it was
def test_constants(lib):
    o = longs(5)
    lib.kl_constants(o)
    assert list(o) == [PLD, 160 * 1024 - 256, 12, 16, PIV]


@pytest.mark.parametrize("F", FRONTS2)
def test_kkt2_offsets_are_the_prefix_sums_of_the_regions(lib, F):
    L = layout2(lib, F)
    at, end = prefix(regions2(F))
    assert {k: L[k] for k in at} == at
    assert L["VAR"] == up(end, 2)
    assert (L["PB"], L["VAR"]) == ANCHORS2[F]
    assert (L["F"], L["FR"], L["PSZ"]) == (F, up(F, 64), (F + 1) * PLD)
    assert (L["NBUF"], L["VP"]) == ((2, 1) if F <= 128 else (1, 0))


@pytest.mark.parametrize("F", FRONTS5)
def test_kkt5_offsets_are_the_prefix_sums_of_the_regions(lib, F):
    L = layout5(lib, F)
    at, end = prefix(regions5(F))
    assert {k: L[k] for k in at} == at
    assert L["PAN"] == up(end, 2) and L["VAR"] == up(L["PAN"] + 4 * (F + 2) * PLD, 2)
    assert (L["PAN"], L["VAR"]) == ANCHORS5[F]
    assert (L["F"], L["FR"], L["PR"], L["PSZ"]) == (F, up(F, 64), F + 2, (F + 2) * PLD)


@pytest.mark.parametrize("F", FRONTS2)
def test_kkt2_byte_counts_equal_the_closed_forms(lib, F):
    for NS, ms, md, nc in GRID:
        s = sizes2(lib, F, NS, ms, md, nc)
        assert s["dbuf_doubles"] == old_kkt2_dbuf(F, md) and s["sbuf_ints"] == old_kkt2_sbuf(F, ms), (NS, ms, md, nc)
        assert s["bytes"] == old_kkt2_lds_bytes(F, NS, ms, md, nc), (NS, ms, md, nc)
        assert s["sweep_base_bytes"] == old_kkt2_sweep_base_bytes(F, NS), (NS, ms, md, nc)
        assert (s["panels3"], s["panels2"], s["records"], s["cells_bytes"], s["fixed"]) == old_two_ended_parts(F, NS, ms, md, nc), (NS, ms, md, nc)


@pytest.mark.parametrize("F", FRONTS5)
def test_kkt5_byte_counts_equal_the_closed_forms(lib, F):
    for NS, ms, md, nc in GRID:
        s = sizes5(lib, F, NS, ms, md, nc)
        assert s["dbuf_doubles"] == old_dma(md, 8) and s["sbuf_ints"] == old_dma(ms, 4), (NS, ms, md, nc)
        assert s["bytes"] == old_kkt5_lds_bytes(F, NS, ms, md, nc), (NS, ms, md, nc)
        assert s["sweep_base_bytes"] == old_kkt5_sweep_base_bytes(F, NS), (NS, ms, md, nc)


def test_sweep_and_chord_byte_counts_equal_the_closed_forms(lib, arena):
    base = arena.ctypes.data
    for NS, steps in itertools.product(NS_GRID, STEP_GRID):
        o = longs(2)
        lib.kl_sweep(NS, steps, C.c_void_p(base), o)
        assert o[1] == old_sweep_ds_lds_bytes(NS, steps), (NS, steps)
        lib.kl_chord(NS, steps, C.c_void_p(base), o)
        assert o[1] == old_chord_lds_bytes(NS, steps), (NS, steps)


# ---------------------------------------------------------------- the carve is sound
def check_sweep(lib, arena, tables_bytes, xp_bytes, base_bytes, NS, live_end_bytes):
    """The sweep's tables at tables_bytes, xp at xp_bytes: behind what the sweep reads, in order, inside base + sweep_ds_lds_bytes."""
    assert tables_bytes >= live_end_bytes
    assert tables_bytes + NS * 12 * 4 <= xp_bytes and xp_bytes % 16 == 0
    assert base_bytes == xp_bytes     # (what lies in front of sweep_ds_lds_bytes is exactly what lies in front of xp)
    for steps in STEP_GRID[1:]:
        o = longs(2)
        lib.kl_sweep(NS, steps, C.c_void_p(arena.ctypes.data + xp_bytes), o)
        rounds = xp_bytes + o[0]
        assert o[0] == NS * PIV * 8 and rounds % 16 == 0
        assert rounds + steps * 16 * 16 <= base_bytes + o[1], (NS, steps)


@pytest.mark.parametrize("F", FRONTS2)
def test_kkt2_carve_is_inside_bytes_in_order_and_aligned(lib, arena, F):
    L = layout2(lib, F)
    base = arena.ctypes.data
    at, _ = prefix(regions2(F))
    size = dict(regions2(F))
    live_end = max(L[k] + size[k] for k in ("UF", "XS", "RED")) * 8
    for NS, ms, md, nc in GRID:
        s = sizes2(lib, F, NS, ms, md, nc)
        assert s["bytes"] <= arena.nbytes
        o = longs(6)
        lib.kl2_carve(F, NS, ms, md, C.c_void_p(base), o)
        dbuf0, sbuf0, hiall, cells, dstride, sstride = o
        nbuf = L["NBUF"]
        assert (dstride, sstride) == (s["dbuf_doubles"], s["sbuf_ints"]) and dstride >= md and sstride >= ms
        # in order and disjoint: every region ends where the next begins or before
        assert dbuf0 == L["VAR"] * 8 and L["VAR"] >= L["PMB"] + (F * PLD if L["VP"] else 0) and L["PMB"] == L["PB"] + 3 * L["PSZ"]
        assert sbuf0 == dbuf0 + nbuf * dstride * 8
        assert hiall == sbuf0 + nbuf * sstride * 4
        assert cells >= hiall + (NS + 1) * 4 and cells == hiall + s["hiall_ints"] * 4
        assert s["cells"] >= nc and cells + s["cells"] * 8 == s["end_bytes"] <= s["bytes"], (NS, ms, md, nc)
        # alignment: the LDS-DMA and the 16-byte accesses of the cells and of xp
        assert dbuf0 % 16 == 0 and sbuf0 % 16 == 0 and cells % 16 == 0
        if nbuf == 2:
            assert (dstride * 8) % 1024 == 0 and (sstride * 4) % 1024 == 0
        assert s["sweep_tables"] == L["PB"]
        check_sweep(lib, arena, s["sweep_tables"] * 8, s["sweep_xp"] * 8, s["sweep_base_bytes"], NS, live_end)
        assert s["sweep_base_bytes"] <= s["bytes"]


@pytest.mark.parametrize("F", FRONTS5)
def test_kkt5_carve_is_inside_bytes_in_order_and_aligned(lib, arena, F):
    L = layout5(lib, F)
    base = arena.ctypes.data
    size = dict(regions5(F))
    live_end = max(L[k] + size[k] for k in ("UF", "XS", "RED")) * 8
    for NS, ms, md, nc in GRID:
        s = sizes5(lib, F, NS, ms, md, nc)
        assert s["bytes"] <= arena.nbytes
        o = longs(3)
        lib.kl5_carve(F, ms, md, C.c_void_p(base), o)
        dbuf, sbuf, cells = o
        assert s["dbuf_doubles"] >= md and s["sbuf_ints"] >= ms
        assert dbuf == L["VAR"] * 8 and L["VAR"] >= L["PAN"] + 4 * L["PSZ"]
        assert sbuf == dbuf + s["dbuf_doubles"] * 8
        assert cells == sbuf + s["sbuf_ints"] * 4
        assert s["cells"] >= nc and cells + s["cells"] * 8 == s["end_bytes"] <= s["bytes"], (NS, ms, md, nc)
        assert dbuf % 16 == 0 and sbuf % 16 == 0 and cells % 16 == 0
        assert (s["dbuf_doubles"] * 8) % 1024 == 0 and (s["sbuf_ints"] * 4) % 1024 == 0
        assert s["sweep_tables"] == L["PAN"]
        check_sweep(lib, arena, s["sweep_tables"] * 8, s["sweep_xp"] * 8, s["sweep_base_bytes"], NS, live_end)
        assert s["sweep_base_bytes"] <= s["bytes"]


def test_chord_xp_and_rounds_are_inside_chord_lds_bytes(lib, arena):
    base = arena.ctypes.data
    for NS, steps in itertools.product(NS_GRID, STEP_GRID):
        o, r = longs(2), longs(2)
        lib.kl_chord(NS, steps, C.c_void_p(base), o)
        xp, total = o
        assert NS * 12 * 4 <= xp and xp % 16 == 0
        if steps == 0:
            assert total == NS * 12 * 4      # (the tables alone: the helper waves are off)
            continue
        lib.kl_sweep(NS, steps, C.c_void_p(base + xp), r)
        assert xp + r[0] + steps * 16 * 16 <= total, (NS, steps)
