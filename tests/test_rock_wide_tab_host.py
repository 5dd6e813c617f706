"""The 16-byte table entries of RockSample's quad loop on the boards with at most eight rocks — host only.

steps_quad_kernel reads one entry {E, M, recA, recB} per lane-step (gym_pomdp_amd/csrc/envs/rock.hip.h: RecWide, its
Tab, build and finish) and keeps the state word in a layout of its own: bit 31 zero, y at bits 28-30, x at 25-27,
rock j's code at bit 5 + 2 j, everything else zero; memory keeps x | y << 4 | codes << 8.  The builder and the lane step are
device code, so both are restated here and run against test_rock_rec_tab_host.py's restatement of the 8-byte form in memory
layout: for every board the form serves — (7,8), (7,7), (4,3), (2,1) — every (action, cell of the board, code of the rock the
step is about, reading) must give the same record and, converted back, the same next state.  The layout's own conditions are
checked on every entry: no bit of M outside a real field lies over a set bit of E, the address needs no mask, the table is
not larger than the 8-byte one."""
import numpy as np
import pytest

from gym_pomdp_amd import tables
from test_rock_rec_tab_host import M32, build_rec_tab, rec_finish

X0, Y0, ROCK0, FLAG = 25, 28, 5, 1 << 31
ACTIONS, SLOTS = 13, 128
BOARDS = {"7-8": (7, 8), "7-7": (7, 7), "4-3": (4, 3), "2-1": (2, 1)}


def from_mem(m):
    return ((m & 7) << X0) | ((m & 0x70) << (Y0 - 4)) | ((m >> (8 - ROCK0)) & (0xFFFF << ROCK0))


def to_mem(s):
    return ((s >> X0) & 7) | ((s >> (Y0 - 4)) & 0x70) | ((s & (0xFFFF << ROCK0)) << (8 - ROCK0))


def build_wide(size, K, stoch=False):
    """-> {(a, x, y): (E, M, recA, recB)} as RockEnv<1>::RecWide::build; a CHECK's E (the threshold word) left 0"""
    grid = {}
    for j, c in enumerate(tables.ROCK_CONFIG[size][2]):          # every listed coordinate is stamped, the last one wins
        grid[tuple(c)] = j
    penalty = 0 if stoch else (0x9C << 16) | (1 << 24)
    tab = {}
    for x in range(size):
        for y in range(size):
            for a in range(5 + K):
                E, M, recA = 0, 0, a
                if a < 4:
                    nx, ny = x + (a == 1) - (a == 3), y + (a == 0) - (a == 2)
                    off = X0 if a & 1 else Y0
                    if 0 <= nx < size and 0 <= ny < size:
                        E, M = (nx if a & 1 else ny) << off, 7 << off
                    else:
                        recA |= ((0x0A << 16) | (1 << 24)) if a == 1 else penalty
                    recB = recA
                elif a == 4:
                    j = grid.get((x, y), -1)
                    if 0 <= j < K:
                        off = ROCK0 + 2 * j
                        E, M = 1 << off, (3 << off) | off | FLAG
                    recA |= penalty
                    recB = recA
                else:
                    M = ROCK0 + 2 * (a - 5)
                    recB = recA | 1 << 8
                    recA |= 2 << 8
                tab[a, x, y] = (E, M, recA, recB)
    return tab


def finish_wide(entry, s, correct, fresh):
    """RockEnv::RecWide::finish -> (record, new state)"""
    E, M, recA, recB = entry
    q = (s >> (M & 31)) & 3
    ok = bool(M >> 31) and q != 1
    rfb = recA if (q != 2) != correct else recB
    rec = (0x00F60004 - q * 0x00760000) & M32 if ok else rfb
    moved = (E & M) | (s & ~M & M32)                             # v_bfi_b32
    return rec, (fresh if rec >= 1 << 24 else moved)


def address(a, s):
    return ((a << 32 | s) >> (X0 - 4)) & M32                     # v_alignbit_b32(a, s, 21)


@pytest.mark.parametrize("board", list(BOARDS))
def test_wide_entries_meet_the_layouts_conditions(board):
    size, K = BOARDS[board]
    assert 5 + K <= ACTIONS and ACTIONS * SLOTS * 16 <= 17 * 256 * 8
    fields = (7 << X0) | (7 << Y0) | (((1 << 2 * K) - 1) << ROCK0)
    seen = set()
    for (a, x, y), (E, M, recA, recB) in build_wide(size, K).items():
        assert M & ~(fields | 31 | FLAG) == 0, (a, x, y)
        assert E & M & ~fields == 0 and E & ~M == 0, (a, x, y)   # (a CHECK's E is its threshold: M's fields are empty there)
        assert (recA & 0xFF) == (recB & 0xFF) == a and (recA == recB or a > 4), (a, x, y)
        s = from_mem(x | y << 4 | 0xFFFF << 8)                   # every code bit set: nothing reaches the address
        ad = address(a, s)
        assert ad == (a * SLOTS + (x | y << 3)) * 16 and ad + 16 <= ACTIONS * SLOTS * 16, (a, x, y)
        seen.add(ad)
        assert s >> 31 == 0 and s & 31 == 0 and (s >> 21) & 15 == 0
    assert len(seen) == size * size * (5 + K)


@pytest.mark.parametrize("board", list(BOARDS))
def test_layout_round_trips_every_state_of_the_board(board):
    size, K = BOARDS[board]
    codes = np.arange(1 << 2 * K, dtype=np.uint64)
    for x in range(size):
        for y in range(size):
            m = np.uint64(x | y << 4) | codes << np.uint64(8)
            s = from_mem(m)
            assert np.all(s >> np.uint64(31) == 0) and np.all(s & np.uint64(0x01E0001F) == 0)
            assert np.all((s >> np.uint64(X0)) & np.uint64(63) == (x | y << 3))
            assert np.array_equal((s >> np.uint64(ROCK0)) & np.uint64(0xFFFF), codes)
            assert np.array_equal(to_mem(s), m)


@pytest.mark.parametrize("stoch", [False, True], ids=["rock", "stochrock"])
@pytest.mark.parametrize("board", list(BOARDS))
def test_wide_step_is_the_step_of_the_8_byte_form(board, stoch):
    """every (cell, action) x every code of the rock the step is about (the others random) x both readings"""
    size, K = BOARDS[board]
    old = build_rec_tab(size, tables.ROCK_CONFIG[size][2][:K], False, 24)
    wide = build_wide(size, K, stoch)
    assert len(old) == len(wide) == size * size * (5 + K)
    rng = np.random.RandomState(16)
    n = 0
    for (a, pos), (e, f) in old.items():
        if stoch and (e >> 28 & 7) == 1:                         # StochasticRock: the penalty is no reward and ends nothing
            e, f = e ^ (7 << 28), f & ~((0xFF << 16) | (1 << 24))
        entry = wide[a, pos & 15, pos >> 4]
        about = (f & 31) - 8 if a >= 4 and (a > 4 or e >> 31) else None
        for code in (0, 1, 2):
            codes = sum(int(c) << (2 * j) for j, c in enumerate(rng.randint(0, 3, K)))
            if about is not None:
                codes = (codes & ~(3 << about)) | (code << about)
            s = pos | codes << 8
            fresh = 0x30 | (int(rng.randint(0, 1 << 16)) & 0xAAAA & ((1 << 2 * K) - 1)) << 8
            for correct in (False, True):
                rec_m, s_m = rec_finish(e, f, s, a, correct, fresh)
                rec_w, s_w = finish_wide(entry, from_mem(s), correct, from_mem(fresh))
                assert rec_w == rec_m and to_mem(s_w) == s_m and from_mem(s_m) == s_w, (board, a, pos, code, correct)
                n += 1
    assert n == size * size * (5 + K) * 6
