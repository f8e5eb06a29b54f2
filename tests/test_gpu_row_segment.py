"""The shared addressing of the window kernels on the MI355X (pytest -m gpu): k_stitch, k_joint_rows, k_track and k_rollout put
the rows of a segment at ring rows (cursor + j) % capacity, the one rule of csrc/row_segment.hpp, which tests/test_row_segment_cpu.py
holds to its definition on the host.  Here every kernel is held to itself: a written ring row equals, to the bit, the same
kernel's table-mode row of the same row number (k_stitch has no table mode: the rows of k_sample, which it repeats to the bit), so
no tolerance comes in; table mode is held to the numpy statements by the kernels' own tests.

Shapes.  B = 3 windows of the reference_compat golden plan at 200 Hz from row 40.  Two capacities: 7, below one wave, so the
wrap falls inside a tile (and the one-wave instantiations run); tile + 3, 515 for the 512-lane kernels and 259 for the rollout's
256, so a window has more than one tile.  Cursors -5 (negative), 0 and capacity * 10^6 + capacity - 2 (two rows in front of
the wrap); per-window counts 0 (the window is not touched and keeps what it carries), capacity + 4 (clamped: exactly capacity
rows) and 3.  With these cursors the only window of more than one tile starts at ring row 0 and the wrap of window 2 lies in
its first tile, so the wide capacity runs once more with window 1's cursor at capacity - 2: its first tile wraps two rows in,
and its second tile starts behind the wrap (the base of a tile at j0 > 0 wrapped).  The rings come pre-filled with a sentinel,
and every row no lane writes still holds it."""
import numpy as np
import pytest

from conftest import load_gv

pytestmark = pytest.mark.gpu
B, HZ, FIRST = 3, 200.0, 40
T0 = np.array([3.756, 0.0, 11.25])
SENT, ISENT = -7.5, -7
COUNT_IN = np.array([[5, 2], [0, 0], [1, 0]], np.int64)
TOTAL_IN = np.array([[1.5, 2.5], [0.0, 0.0], [0.25, 0.5]])
WIDE, ROLLOUT_WIDE = 512 + 3, 256 + 3


def cursors(cap, mid=0):
    return np.array([-5, mid, cap * 10 ** 6 + cap - 2], np.int64)


def counts(cap):
    return np.array([0, cap + 4, 3], np.int32)


def places(cap, mid=0):
    """Per window the ring rows of its segment, spelled here: (cursor + j) % capacity for j below the clamped count."""
    return [(int(c) + np.arange(min(int(n), cap))) % cap for c, n in zip(cursors(cap, mid), counts(cap))]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and (np.array_equal(a.view(np.int64), b.view(np.int64)) if a.dtype == np.float64 else np.array_equal(a, b))


def check_ring(ring, table, cap, sentinel, mid=0):
    """ring [B, cap, ...] against table [B, cap, ...], whose row j is the segment's row j."""
    for b, at in enumerate(places(cap, mid)):
        assert len(at) == (0, cap, 3)[b] and len(set(at.tolist())) == len(at)
        assert same(ring[b, at], table[b, :len(at)]), b
        free = np.setdiff1d(np.arange(cap), at)
        assert len(free) == cap - len(at) and (ring[b, free] == sentinel).all(), b


@pytest.fixture(scope="module")
def win(cfg):
    """The planner, the windows' nodes, and per capacity the table-mode joint rows and the measured rows on the plan."""
    from qtos_amd import capi
    from qtos_amd.capi import Planner

    class Windows:
        pass
    w = Windows()
    w.cfg, w.P = cfg, Planner(cfg, max_batch=8)
    w.nodes = np.repeat(np.array(load_gv("gv1")["x"])[None], B, axis=0)
    w.joint, w.meas, w.plan = {}, {}, {}
    rng = np.random.default_rng(43)
    for cap in (7, ROLLOUT_WIDE, WIDE):
        w.plan[cap] = w.P.sample(w.nodes, T0, hz=HZ, n_rows=FIRST + cap)[:, FIRST:]
        w.joint[cap], _ = w.P.joint_rows(w.nodes, T0, capi.joint_params(hz=HZ, first_row=FIRST, n_rows=cap, tau_max=0.0))
        w.meas[cap] = np.concatenate([w.plan[cap][:, :, 1:7], w.joint[cap][:, :, 1:13]], 2) + 1e-3 * rng.standard_normal((B, cap, 18))
    yield w
    w.P.close()


def ring_of(table, cap, fill, mid=0):
    """A ring that holds the table's row j of every window at the window's place of row j, `fill` elsewhere."""
    ring = np.full(table.shape, fill, table.dtype)
    for b, at in enumerate(places(cap, mid)):
        ring[b, at] = table[b, :len(at)]
    return ring


@pytest.mark.parametrize("cap, mid", [(7, 0), (WIDE, 0), (WIDE, WIDE - 2)])
def test_stitch(win, cap, mid):
    held = np.minimum(counts(cap), cap)
    traj, cursor, t0 = win.P.stitch(win.nodes, counts(cap), T0, np.full((B, cap, 37), SENT), cursors(cap, mid), first_row=FIRST, hz=HZ)
    check_ring(traj, win.plan[cap], cap, SENT, mid)
    assert cursor.tolist() == [int(c) + int(n) for c, n in zip(cursors(cap, mid), held)]
    assert same(t0, T0 + held.astype(np.float64) / HZ) and same(t0[:1], T0[:1])            # window 0: its cursor and clock as they came


@pytest.mark.parametrize("cap, mid", [(7, 0), (WIDE, 0), (WIDE, WIDE - 2)])
def test_joint_rows(win, cap, mid):
    from qtos_amd import capi
    kw = dict(hz=HZ, first_row=FIRST, tau_max=0.0)
    t_out, t_st = win.P.joint_rows(win.nodes, T0, capi.joint_params(n_rows=cap, **kw), n_rows=counts(cap))
    out, st = win.P.joint_rows(win.nodes, T0, capi.joint_params(capacity=cap, **kw), n_rows=counts(cap), cursor=cursors(cap, mid),
                               out=np.full((B, cap, 37), SENT), status=np.full((B, cap), ISENT, np.int32))
    check_ring(out, t_out, cap, SENT, mid)
    check_ring(st, t_st, cap, ISENT, mid)


@pytest.mark.parametrize("cap, mid", [(7, 0), (WIDE, 0), (WIDE, WIDE - 2)])
def test_track(win, cap, mid):
    from qtos_amd import capi
    kw = dict(hz=HZ, first_row=FIRST, delay=3)
    acc = dict(n_rows=counts(cap), count=COUNT_IN, total=TOTAL_IN)
    t_out, t_st, t_count, t_total = win.P.track(win.nodes, T0, win.meas[cap], capi.track_params(n_rows=cap, **kw), **acc)
    out, st, count, total = win.P.track(win.nodes, T0, ring_of(win.meas[cap], cap, SENT, mid), capi.track_params(capacity=cap, **kw),
                                        cursor=cursors(cap, mid), out=np.full((B, cap, 26), SENT), status=np.full((B, cap), ISENT, np.int32), **acc)
    check_ring(out, t_out, cap, SENT, mid)
    check_ring(st, t_st, cap, ISENT, mid)
    assert same(count, t_count) and same(total, t_total)
    assert same(count[0], COUNT_IN[0]) and same(total[0], TOTAL_IN[0])                     # window 0 keeps its accumulators
    assert count[1:, 0].tolist() == [cap, 1 + 3]


@pytest.mark.parametrize("cap, mid", [(7, 0), (ROLLOUT_WIDE, 0), (ROLLOUT_WIDE, ROLLOUT_WIDE - 2)])
def test_rollout(win, cap, mid):
    from qtos_amd import capi
    from rollout_cases import body_kw
    kw = dict(cfg=win.cfg, hz=HZ, first_row=FIRST, init=True, **body_kw("held", 1))
    state_in = np.arange(1.0, 1.0 + B * 13).reshape(B, 13)
    carried = dict(n_rows=counts(cap), state=state_in, count=np.array([5, 0, 2], np.int64), word=np.array([32, 0, 0], np.int32))
    t_meas, t_rows, t_st, t_state, t_count, t_word = win.P.rollout(win.nodes, T0, capi.rollout_params(n_rows=cap, **kw),
                                                                   joint=win.joint[cap], **carried)
    meas, rows, st, state, count, word = win.P.rollout(
        win.nodes, T0, capi.rollout_params(capacity=cap, **kw), cursor=cursors(cap, mid), joint=ring_of(win.joint[cap], cap, np.nan, mid),
        meas=np.full((B, cap, 18), SENT), rows=np.full((B, cap, 20), SENT), status=np.full((B, cap), ISENT, np.int32), **carried)
    check_ring(meas, t_meas, cap, SENT, mid)
    check_ring(rows, t_rows, cap, SENT, mid)
    check_ring(st, t_st, cap, ISENT, mid)
    assert same(state, t_state) and same(count, t_count) and same(word, t_word)
    assert same(state[0], state_in[0]) and count.tolist() == [5, cap, 2 + 3] and word[0] == 32   # window 0 keeps state, count and word
