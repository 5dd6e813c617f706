"""The rotated state layout of RockSample's quad loops at its edges — host only.

steps_quad_kernel keeps a one-word state rotated right by 8 in registers: rock j's code at bits 2 j, 2 j + 1, the position
byte on top at bits 24-31 (RockEnv::ROT_POS in gym_pomdp_amd/csrc/envs/rock.hip.h); memory keeps x | y << 4 | codes << 8.
The table builder is device code, so its packing (rec_f, build_rec_tab, Rec8::finish) is restated here for both layouts and the
two are run against each other: a step in the rotated layout must be the rotation of the step in memory layout, for every
cell, action, rock code and reading — in particular for the last rock of a 12-rock board, whose code sits right under the
position byte, where a carry out of `s + (c << off)` would move the agent.

The position byte cannot sit at bits 16-23 with the codes below it: 11 rocks need 22 bits and 12 need 24, so the bounds
checked are the layout's own: every rock offset + 2 <= ROT_POS = 24, every move offset ROT_POS or ROT_POS + 4."""
import os
import re

import numpy as np
import pytest

from gym_pomdp_amd import tables

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym_pomdp_amd", "csrc", "envs", "rock.hip.h")
REC_LUT = 0x000000000A0A9CF6                       # reward byte by outcome code (REC_LUT_HI : REC_LUT_LO)
NOTHING, PENALTY, EXIT_EAST, NO_TIE = 6 << 28, 1 << 28, 3 << 28, 1 << 27
M32 = 0xFFFFFFFF


def rot_pos():
    m = re.search(r"ROT_POS\s*=\s*(\d+)u;", open(HEADER).read())
    assert m, "RockEnv::ROT_POS not found"
    return int(m.group(1))


def rotr(s, r):
    return ((s >> r) | (s << (32 - r))) & M32


def rec_f(off, c, ob_mask, oc):
    return off | ((c & 3) << 5) | (ob_mask << 8) | (((REC_LUT >> (8 * oc)) & 0xFF) << 16) | ((oc & 1) << 24)


def build_rec_tab(size, rocks, rot, pos0):
    """-> {(a, pos): (e, f)} as RockEnv<1>::build_rec_tab<POS0> (rot: POS0 = ROT_POS, else 0); the CHECK entries' thresholds left out (e = NOTHING)"""
    K = len(rocks)
    grid = {(x, y): j for j, (x, y) in enumerate(rocks)}
    p0, r0 = (pos0, 0) if rot else (0, 8)
    tab = {}
    for x in range(size):
        for y in range(size):
            pos = x | y << 4
            for a in range(5 + K):
                if a < 4:
                    nx, ny = x + (a == 1) - (a == 3), y + (a == 0) - (a == 2)
                    inside = 0 <= nx < size and 0 <= ny < size
                    e = (((pos ^ (nx | ny << 4)) | NOTHING) if inside else (EXIT_EAST if a == 1 else PENALTY)) | NO_TIE
                    f = rec_f(p0 + (0 if a & 1 else 4), (1 if a < 2 else -1) if inside else 0, 0, e >> 28 & 7)
                elif a == 4:
                    j = grid.get((x, y), -1)
                    e = ((8 + 2 * j) | 0x80000000 if j >= 0 else 0) | PENALTY | NO_TIE
                    f = rec_f(r0 + 2 * j if j >= 0 else 0, 0, 0, e >> 28 & 7)
                else:
                    e = NOTHING
                    f = rec_f(r0 + 2 * (a - 5), 0, 3, 6)
                tab[a, pos] = (e, f)
    return tab


def rec_finish(e, f, s, a, correct, fresh):
    """RockEnv::Rec8::finish -> (record, new state)"""
    off = f & 31
    q = (s >> off) & 3
    ok = bool(e >> 31) and q != 1
    keep = 0xFFFFFE00 if (q == 2) == correct else 0xFFFFFD00
    rec = (0x00F60004 - q * 0x00760000) & M32 if ok else (f & keep) | a
    c = 1 - q if ok else ((f >> 5) & 3) - 4 * ((f >> 6) & 1)
    moved = (s + (c << off)) & M32
    return rec, (fresh if rec >= 1 << 24 else moved)


TWELVE = (15, tables.ROCK_CONFIG[15][2][:12])       # the 12-rock parameter block: RockSample(15,15)'s first twelve rocks
BOARDS = {"2-1": (2, tables.ROCK_CONFIG[2][2]), "7-8": (7, tables.ROCK_CONFIG[7][2]), "11-11": (11, tables.ROCK_CONFIG[11][2]),
          "12 rocks": TWELVE}


@pytest.mark.parametrize("board", list(BOARDS))
def test_rotated_table_offsets_stay_in_their_fields(board):
    size, rocks = BOARDS[board]
    P = rot_pos()
    assert P == 24 and 2 * 12 <= P
    for (a, pos), (e, f) in build_rec_tab(size, rocks, True, P).items():
        off = f & 31
        if a < 4:
            assert off in (P, P + 4), (a, pos, off)
        else:
            assert off + 2 <= P, (a, pos, off)
    for (a, pos), (e, f) in build_rec_tab(size, rocks, False, P).items():      # ... and memory layout keeps its own
        off = f & 31
        assert (off in (0, 4)) if a < 4 else (off == 0 or 8 <= off <= 30), (a, pos, off)


@pytest.mark.parametrize("board", list(BOARDS))
def test_rotated_step_is_the_rotation_of_the_step(board):
    """every (cell, action) of the board x every code of the rock the step is about (the others random) x both readings:
    record equal, state equal after rotating back — no carry leaves a field in either layout"""
    size, rocks = BOARDS[board]
    P, K = rot_pos(), len(rocks)
    mem, rot = build_rec_tab(size, rocks, False, P), build_rec_tab(size, rocks, True, P)
    rng = np.random.RandomState(13)
    for (a, pos), (e, f) in mem.items():
        er, fr = rot[a, pos]
        assert e == er and (f ^ fr) < 32                                     # only the offsets differ
        about = (f & 31) - 8 if a >= 4 and (a > 4 or e >> 31) else None          # bit offset (within the codes) of the rock the step reads
        for code in (0, 1, 2):
            codes = sum(int(c) << (2 * j) for j, c in enumerate(rng.randint(0, 3, K)))
            if about is not None:
                codes = (codes & ~(3 << about)) | (code << about)
            s = pos | codes << 8
            fresh = 0x30 | (int(rng.randint(0, 1 << 24)) & 0xAAAAAA & ((1 << 2 * K) - 1)) << 8
            for correct in (False, True):
                rec_m, s_m = rec_finish(e, f, s, a, correct, fresh)
                rec_r, s_r = rec_finish(er, fr, rotr(s, 8), a, correct, rotr(fresh, 8))
                assert rec_m == rec_r and rotr(s_m, 8) == s_r, (board, a, pos, code, correct)
                assert (s_m & 0xFF) == (s_r >> P) and s_m >> (8 + 2 * K) == 0


def test_twelfth_rock_never_reaches_the_position_byte():
    """the last rock of a 12-rock board at bits 22-23 of the rotated word, the agent at (15, 15) above it and on the rock's own
    cell below: collecting it (code 0 -> 1: + 1 << 22, code 2 -> 1: - 1 << 22) leaves the position byte alone"""
    P = rot_pos()
    e, f = NO_TIE | PENALTY | 0x80000000 | (8 + 22), rec_f(22, 0, 0, 1)
    for pos in (0xFF, 0x19, 0x00):
        for code in (0, 2):
            for low in (0, (1 << 22) - 1):
                s = pos << P | code << 22 | low
                rec, s2 = rec_finish(e, f, s, 4, False, 0)
                assert s2 == (pos << P | 1 << 22 | low) and rec == ((0x00F60004, None, 0x000A0004)[code])


def test_alignbit_round_trips_every_twelve_rock_state_at_the_far_corner():
    """v_alignbit_b32(s, s, 8) after the launch's load, v_alignbit_b32(s, s, 24) before its store: every word with position
    (15, 15) and 24 bits of codes comes back as it was, with the codes from bit 0 and the position on top in between"""
    codes = np.arange(1 << 24, dtype=np.uint32)
    s = np.uint32(0xFF) | (codes << np.uint32(8))
    r = (s >> np.uint32(8)) | (s << np.uint32(24))                              # alignbit(s, s, 8)
    assert np.array_equal(r & np.uint32(0xFFFFFF), codes) and np.all(r >> np.uint32(24) == 0xFF)
    back = (r >> np.uint32(24)) | (r << np.uint32(8))                           # alignbit(r, r, 24)
    assert np.array_equal(back, s)
