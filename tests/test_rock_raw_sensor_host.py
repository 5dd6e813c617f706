"""RockSample's one-state-word table entry since the lane step compares the RAW sensor word, and the numeric reset-tie filter —
host only.

The entry's first word is what the lane's sensor high word H compares with (gym_pomdp_amd/csrc/envs/rock.hip.h): a CHECK
stores E = T << 5 with T = thr >> 26, saturated to 0xFFFFFFFF where T = 2^27 (the always-right sensor at distance 0), every
other entry 0xFFFFFFFF; the rock-under-a-SAMPLE flag sits in bit 31 of the second word.  `correct` = H < E on the common path;
a lane with H - E < 32 (unsigned) recomputes the draw from the threshold itself (Rec8::exact).  The packing is device
code, so it is restated here and held against the definition it replaces — (H >> 5) < T, or the low word against the
threshold's low 26 bits when (H >> 5) == T — and against test_rock_rec_tab_host.py's restatement of the old entry.

fresh_words' filter for K <= RESET_NUMERIC_K rocks is numeric: a tied rock j means rotr(w, 2 j + 2) in [2^31, 2^31 + 32), so
bit 2 j + 1 and bits 2 j + 2 .. 2 j + 6 are the only ones that may be set: w < 2^(2 K + 5)."""
import os
import re

import numpy as np
import pytest

from gym_pomdp_amd import tables
from test_rock_rec_tab_host import BOARDS, HEADER, M32, build_rec_tab, rec_f, rot_pos, rotr
from test_rock_rec_tab_host import rec_finish as rec_finish_old

LO_MASK = (1 << 26) - 1
REC_ROCK = 1 << 31
TIE_SPAN = 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def header_const(name):
    m = re.search(name + r"\s*=\s*(\d+)u?;", open(HEADER).read())
    assert m, "RockEnv::%s not found" % name
    return int(m.group(1))


def rec_thr_word(T):
    """RockEnv::rec_thr_word (RecWide::thr_word keeps the low five bits of the saturated word clear)"""
    return M32 if T >= 1 << 27 else T << 5


def old_decision(H, L, thr):
    """the definition the raw compare replaces (RockEnv::k53_le on the sensor's double)"""
    kh, T = H >> 5, thr >> 26
    return (L >> 6) <= (thr & LO_MASK) if kh == T else kh < T


def new_decision(H, L, thr, E):
    """the common compare, patched by the rare path whenever H - E < TIE_SPAN (RockEnv::Rec8::exact)"""
    correct = H < E
    if (H - E) & M32 < TIE_SPAN:
        kh, T = H >> 5, thr >> 26
        correct = (L >> 6) <= (thr & LO_MASK) if kh == T else kh < T
    return correct


def rec_finish_new(f, s, a, correct, fresh):
    """RockEnv::Rec8::finish with the flag in the second word -> (record, new state)"""
    off = f & 31
    q = (s >> off) & 3
    ok = bool(f >> 31) and q != 1
    keep = 0x7FFFFE00 if (q == 2) == correct else 0x7FFFFD00
    rec = (0x00F60004 - q * 0x00760000) & M32 if ok else (f & keep) | a
    c = 1 - q if ok else ((f >> 5) & 3) - 4 * ((f >> 6) & 1)
    moved = (s + (c << off)) & M32
    return rec, (fresh if rec >= 1 << 24 else moved)


def sensor_words(E, thr):
    """the sensor words the issue names around an entry E, and low words on both sides of the threshold's low part"""
    tl = thr & LO_MASK
    Hs = sorted({(E - 1) & M32, E, (E + 31) & M32, (E + 32) & M32, 0, M32})
    Ls = sorted({0, (tl << 6) & M32, ((tl << 6) + 63) & M32, ((tl + 1) << 6) & M32, M32})
    return Hs, Ls


def thr_at(d):
    return int(tables.ROCK_THR[min(d, len(tables.ROCK_THR) - 1)])


@pytest.mark.parametrize("board", list(BOARDS))
def test_raw_compare_and_rare_path_equal_the_old_definition(board):
    """every cell, every CHECK: H at E - 1, E, E + 31, E + 32, 0 and 0xFFFFFFFF, the low word on both sides of the threshold's"""
    size, rocks = BOARDS[board]
    saturated = unsaturated = 0
    for x in range(size):
        for y in range(size):
            for rx, ry in rocks:
                thr = thr_at(abs(x - rx) + abs(y - ry))
                T = thr >> 26
                assert T <= 1 << 27
                E = rec_thr_word(T)
                saturated += T == 1 << 27
                unsaturated += T < 1 << 27
                assert (E == M32) == (T == 1 << 27) and (T == 1 << 27 or E >> 5 == T)
                Hs, Ls = sensor_words(E, thr)
                for H in Hs:
                    for L in Ls:
                        assert new_decision(H, L, thr, E) == old_decision(H, L, thr), (board, x, y, hex(H), hex(L), hex(thr))
    assert saturated and unsaturated, board                              # a cell on a rock, a cell away from one


def test_every_threshold_of_the_table_and_the_edges_of_T():
    """every threshold the env's table holds, and T = 0, 1, 2^26, 2^27 - 1 (unsaturated, E = 0xFFFFFFE0) and 2^27 (saturated)"""
    thrs = [int(t) for t in tables.ROCK_THR] + [T << 26 | lo for T in (0, 1, 1 << 26, (1 << 27) - 1) for lo in (0, 12345, LO_MASK)] + [1 << 53]
    assert any(t >> 26 == 1 << 27 for t in thrs) and any(t >> 26 < 1 << 27 for t in thrs)
    for thr in thrs:
        E = rec_thr_word(thr >> 26)
        Hs, Ls = sensor_words(E, thr)
        for H in Hs + list(range(0, 70)) + list(range(M32 - 70, M32 + 1)):
            for L in Ls:
                assert new_decision(H, L, thr, E) == old_decision(H, L, thr), (hex(thr), hex(H), hex(L))
    # off the filter the compare alone is exact: a sweep of H around an unsaturated entry
    thr = thr_at(3)
    E = rec_thr_word(thr >> 26)
    for H in range(E - 200, E + 200):
        if (H - E) & M32 >= TIE_SPAN:
            assert (H < E) == old_decision(H, 0, thr) == old_decision(H, M32, thr)


@pytest.mark.parametrize("board", list(BOARDS))
def test_non_check_entries_and_the_flag_bit(board):
    """A move's or a SAMPLE's entry holds 0xFFFFFFFF: the filter passes it only at H = 0xFFFFFFFF and H < 31 (2^-27 per
    lane-step), and whatever the rare path then says, the record and the state are those of the old entry.  With the flag bit set in the second word every record's
    byte 3 is still 0 or 1, in both layouts."""
    size, rocks = BOARDS[board]
    P, K = rot_pos(), len(rocks)
    rng = np.random.RandomState(5)
    flagged = 0
    for rot in (False, True):
        for (a, pos), (e, f) in build_rec_tab(size, rocks, rot, P).items():
            E = rec_thr_word(thr_at(0) >> 26) if a > 4 else M32               # (a CHECK's threshold does not matter here)
            fn = f | (e & REC_ROCK if a == 4 else 0)
            flagged += fn >> 31
            if a <= 4:                                                        # the filter wraps: 0xFFFFFFFF itself and the 31 words after it
                near = [H for H in (0, 1, 30, 31, 32, 1 << 31, E - 33, E - 32, E - 1, E) if (H - E) & M32 < TIE_SPAN]
                assert near == [0, 1, 30, M32]
            for code in (0, 1, 2):
                codes = sum(int(c) << (2 * j) for j, c in enumerate(rng.randint(0, 3, K)))
                s = (pos << P | codes) if rot else (pos | codes << 8)
                if a >= 4:
                    off = fn & 31
                    s = (s & ~(3 << off)) | (code << off)
                fresh = 0x12345678
                recs = set()
                for correct in (False, True):
                    rec, s2 = rec_finish_new(fn, s, a, correct, fresh)
                    assert (rec >> 24) in (0, 1), (board, a, pos, hex(rec))
                    assert (rec, s2) == rec_finish_old(e, f, s, a, correct, fresh), (board, rot, a, pos, code, correct)
                    recs.add((rec, s2))
                assert a > 4 or len(recs) == 1, (board, a, pos)               # the rare path cannot change a non-CHECK's record
    assert flagged == 2 * len(set(rocks))


def rotl(w, r):
    r &= 31
    return ((w << r) | (w >> (32 - r))) & M32 if r else w


def popc(w):
    return bin(w).count("1")


def filter_passes(words, K, numeric_k):
    """RockEnv::fresh_words' way into the tie branch (the filters of RecWide::fresh / Rec8::fresh) for one thread's words (four of a quad, two of half a quad)"""
    if K <= numeric_k:
        return min(words) < 1 << (2 * K + 5)
    return min(popc(w) for w in words) <= 6


def test_numeric_reset_filter_never_skips_a_tie():
    numeric_k = header_const("RESET_NUMERIC_K")
    assert numeric_k == 8
    rng = np.random.RandomState(11)
    for K in range(1, 13):
        assert 2 * K + 5 < 32
        for j in range(K):
            for x in range(32):
                w = rotl(1 << 31 | x, 2 * j + 2)
                assert rotr(w, 2 * j + 2) >> 5 == 1 << 26                    # rock j of this word ties
                assert w < 1 << (2 * K + 5), (K, j, x)
                assert popc(w) <= 6                                          # ... and the test inside the branch finds it
                for N in (4, 2):
                    others = [int(v) for v in rng.randint(0, 1 << 32, N - 1, dtype=np.uint64)]
                    for at in range(N):
                        words = others[:at] + [w] + others[at:]
                        assert filter_passes(words, K, numeric_k), (K, j, x, N, at)   # the arm this K takes
                        assert filter_passes(words, K, 0) and filter_passes(words, K, 12)   # ... and the other one too


def test_reset_tie_fixture_words_pass_the_filter():
    """the lanes of ties_rock_auto.npz: the word their fresh episode starts from (the step's sensor block at t = 1) has a rock
    on the 2^52 boundary, is below 2^(2 K + 5) for RockSample(7,8)'s K = 8 and has at most six bits set"""
    from oracle import philox_ref as px
    g = dict(np.load(os.path.join(GOLDEN, "ties_rock_auto.npz")))
    seed, K = int(g["seed"]), 8
    for lane, j in zip(g["lanes"], g["tied_rock"]):
        words = px.rock_reset_words(seed, int(lane), 1, K, auto_step_block=0)
        w = rotl(int(words[0]), 2)                                           # rock 0's high word is the lane's word rotated right by 2
        assert rotr(w, 2 * int(j) + 2) >> 5 == 1 << 26, (lane, j)
        assert w < 1 << (2 * K + 5) and popc(w) <= 6, (lane, hex(w))
        assert filter_passes([w, M32, M32, M32], K, header_const("RESET_NUMERIC_K"))
