"""The three ways the project builds a BattleShip board (gym_pomdp_amd/csrc/envs/battleship.hip.h), restated in plain Python and
compared with the CPU oracle's boards, without a GPU.  Masks are Python integers cut to the kernel's mask type (32, 64 or 128
bits), oracle/philox_ref.py supplies the words of streams RESET and NEXT.

    board_sequential    board(): one ship after the other, position word(s) then a direction word
    Builder / feed      the two-state word consumer of the fused loops' builder pool (feed), and feed2 — two words at once with
                        one placement test — which the pool calls twice per Philox block
    board_windowed      reset_where(): 64-word windows, direction_words(A) assigns the roles, the lowest successful candidate
                        is the ship, the cursor stops before an accepted position word that is the window's last word

Boards: the table of tests/test_gpu_battleship_boards.py (every mask width, masks filled to the last bit, 1-, 2- and 16-wide
boards), 256 lanes each: `occ` and `next` after batch_reset, `next` again after one forced episode end.

The file can fail.  Each of these one-token changes of the restatement was run once (none is committed):
    blocked_of: `shr_small(occ | e1, X, mw)` -> `shr_small(h, X, mw)` (looks at NW as well)
        test_blocked_of_is_the_eight_neighbours_minus_nw fails on every board wider than one cell ((2, 13), lone cell (0, 1):
        blocked 63, wanted 61) and test_builders_equal_the_oracle on ten of the eleven boards ((1, 16) has no NW neighbour)
    feed2: `(w0 if D else w1) & 3` -> `(w1 if D else w0) & 3` (the two words swapped where the direction is read)
        test_feed2_equals_two_feeds and test_builders_equal_the_oracle fail on every board, the latter on lane 0's first board
    board_windowed: `cur += nv - 1 if last_is_position else nv` -> `cur += nv` (consumes the window's last accepted position)
        test_the_cursor_stops_before_an_accepted_position_at_the_windows_end fails for every stream ((8651809, 70) against
        (25633, 75): another board, another cursor) and test_builders_equal_the_oracle on eight boards
"""
import numpy as np
import pytest

from oracle import philox_ref as pr

# (X, Y), max_len — the boards of tests/test_gpu_battleship_boards.py
BOARDS = [((2, 13), 3), ((13, 2), 3), ((1, 16), 3), ((8, 6), 4), ((8, 8), 4), ((9, 10), 5), ((6, 15), 5), ((10, 10), 5), ((16, 7), 5),
          ((7, 16), 5), ((16, 7), 7)]
IDS = ["%dx%d-%d" % (b + (m,)) for b, m in BOARDS]
SEED, LANE0, T0, LANES, NWORDS = 0x9E3779B97F4A7C15, (1 << 22) + 8, (1 << 32) - 3, 256, 4096
COMPASS = [(0, 1), (1, 0), (0, -1), (-1, 0)]                       # N E S W (battleship.py:12-21)


def mask_words(X, Y):
    return (X * Y + 6 + 31) // 32


def mbits(mw):
    return 32 if mw == 1 else 64 if mw == 2 else 128


def shl_small(a, s, mw):
    """1 <= s <= 63 (X == 1 .. 16); 128 bits: two 64-bit halves as the kernel writes them"""
    if mw <= 2:
        return (a << s) & ((1 << mbits(mw)) - 1)
    lo, hi, m64 = a & (2 ** 64 - 1), a >> 64, 2 ** 64 - 1
    return ((lo << s) & m64) | (((((hi << s) & m64) | (lo >> (64 - s))) & m64) << 64)


def shr_small(a, s, mw):
    if mw <= 2:
        return a >> s
    lo, hi, m64 = a & (2 ** 64 - 1), a >> 64, 2 ** 64 - 1
    return ((lo >> s) | ((hi << (64 - s)) & m64)) | ((hi >> s) << 64)


class Consts(object):
    """build_consts(): what the builders derive from the board size"""

    def __init__(self, X, Y, max_len):
        self.X, self.Y, self.cells, self.max_len = X, Y, X * Y, max_len
        self.mw = mask_words(X, Y)
        self.M = (1 << mbits(self.mw)) - 1
        self.rmask = 0xFFFFFFFF >> (32 - ((self.cells - 1) | 1).bit_length())
        self.inv_x = (65536 + X - 1) // X
        self.col0 = sum(1 << (y * X) for y in range(Y)) & self.M
        self.colL = (self.col0 << (X - 1)) & self.M
        self.vpat = [sum(1 << (i * X) for i in range(k)) & (2 ** 128 - 1) & self.M for k in range(12)]


def blocked_of(occ, c):
    """occ and its N, E, S, W, NE, SE, SW shifts (NW excluded): h = {self, E, W}; south side = h << X; north = {self, E} >> X"""
    X, mw = c.X, c.mw
    e1 = (occ & ~c.col0 & c.M) >> 1
    h = occ | e1 | (((occ & ~c.colL) << 1) & c.M)
    return h | shr_small(occ | e1, X, mw) | shl_small(h, X, mw)


def sbfe(src, offset, width):
    v = (src >> offset) & ((1 << width) - 1)
    return v - (1 << width) if v >> (width - 1) else v


def placement(c, blocked, a0, dirword, length):
    """the test of one (position, direction) pair: (fits, stride, dx) with the kernel's arithmetic"""
    dir2 = (dirword & 3) << 1
    dx, dy = sbfe(0xC4, dir2, 2), sbfe(0x31, dir2, 2)
    py = (a0 * c.inv_x) >> 16
    px = a0 - py * c.X
    ex, ey, stride = px + (length + 1) * dx, py + (length + 1) * dy, dy * c.X + dx
    inside = 0 <= ex < c.X and 0 <= ey < c.Y
    lo = a0 if stride > 0 else a0 + length * stride
    pat = (1 << (length + 1)) - 1 if dx != 0 else c.vpat[length + 1]
    test = (pat << (lo & (mbits(c.mw) - 1))) & c.M
    return inside and (test & blocked) == 0, stride, dx


def mark(c, occ, a0, stride, dx, length):
    low = a0 if stride > 0 else a0 + (length - 1) * stride
    return occ | (((((1 << length) - 1) if dx != 0 else c.vpat[length]) << (low & (mbits(c.mw) - 1))) & c.M)


# ---- 1. board(): sequential ----------------------------------------------------------------------------------------------------
def board_sequential(c, words):
    """-> (occ, words consumed)"""
    occ, i = 0, 0
    for length in range(c.max_len, 1, -1):
        blocked = blocked_of(occ, c)
        while True:
            while (words[i] & c.rmask) > c.cells - 1:
                i += 1
            a0, d = words[i] & c.rmask, words[i + 1]
            i += 2
            ok, stride, dx = placement(c, blocked, a0, d, length)
            if ok:
                break
        occ = mark(c, occ, a0, stride, dx, length)
    return occ, i


# ---- 2. the two-state builder --------------------------------------------------------------------------------------------------
class Builder(object):
    def __init__(self, c):
        self.occ, self.blocked, self.len, self.a0, self.want_dir = 0, 0, c.max_len, 0, False

    def key(self):
        return self.occ, self.blocked, self.len, self.a0, self.want_dir

    def live_key(self):
        """what later words can see: a0 is read only while a direction word is awaited (feed2 leaves a rejected w0 in it)"""
        return self.occ, self.blocked, self.len, self.a0 if self.want_dir else None, self.want_dir

    def clone(self):
        b = Builder.__new__(Builder)
        b.occ, b.blocked, b.len, b.a0, b.want_dir = self.key()
        return b


def feed(b, c, w):
    length, a0 = b.len, b.a0
    live = length >= 2
    ok, stride, dx = placement(c, b.blocked, a0, w, length)
    if live and b.want_dir and ok:
        b.occ = mark(c, b.occ, a0, stride, dx, length)
        b.len = length - 1
        b.blocked = blocked_of(b.occ, c)
    v = w & c.rmask
    accept = live and not b.want_dir and v <= c.cells - 1
    b.a0 = v if accept else a0
    b.want_dir = accept


def feed2(b, c, w0, w1):
    length = b.len
    live, D = length >= 2, b.want_dir
    v0, v1 = w0 & c.rmask, w1 & c.rmask
    acc0, acc1 = v0 <= c.cells - 1, v1 <= c.cells - 1
    test_now = live and (D or acc0)
    a0 = b.a0 if D else v0
    ok, stride, dx = placement(c, b.blocked, a0, (w0 if D else w1) & 3, length)
    len_after = length
    if test_now and ok:
        b.occ = mark(c, b.occ, a0, stride, dx, length)
        len_after = b.len = length - 1
        b.blocked = blocked_of(b.occ, c)
    accept1 = len_after >= 2 and (D or not acc0) and acc1
    b.a0 = v1 if accept1 else a0
    b.want_dir = accept1


def board_feed(c, words):
    b, i = Builder(c), 0
    while b.len >= 2:
        feed(b, c, words[i])
        i += 1
    return b.occ, i


def board_feed2(c, words):
    """as the pool runs it: a Philox block is feed2(x, y), feed2(z, w); a finished board is taken at the block's end"""
    b, i = Builder(c), 0
    while b.len >= 2:
        feed2(b, c, words[i], words[i + 1])
        feed2(b, c, words[i + 2], words[i + 3])
        i += 4
    return b.occ


# ---- 3. reset_where(): windowed ------------------------------------------------------------------------------------------------
def direction_words(a):
    m = 2 ** 64 - 1
    even = 0x5555555555555555
    follows = (a << 1) & m
    odd_starts = a & ~even & ~follows & m
    even_start_runs = (odd_starts + a) & m
    return (even ^ ((even_start_runs << 1) & m)) & follows


def sequential_roles(a, nbits=64):
    """D[l] = A[l-1] & ~D[l-1]: the word after an accepted position word is its direction word"""
    d, prev_pos = 0, False
    for l in range(nbits):
        if prev_pos:
            d |= 1 << l
            prev_pos = False
        else:
            prev_pos = bool((a >> l) & 1)
    return d


def board_windowed(c, words, stats=None):
    """-> (occ, cursor after the last ship); stats counts the windows that ended on an accepted position word"""
    occ, cur, c0 = 0, 0, -64
    for length in range(c.max_len, 1, -1):
        blocked = blocked_of(occ, c)
        while True:
            if cur - c0 > 32:
                c0 = cur                                                # the window is words c0 .. c0 + 63
            nv = 64 - (cur - c0)
            A = 0
            for l in range(nv):
                if (words[cur + l] & c.rmask) <= c.cells - 1:
                    A |= 1 << l
            D = direction_words(A)
            cand = A & ~D & ((1 << (nv - 1)) - 1)
            placed = False
            l = 0
            while cand >> l:
                if (cand >> l) & 1:
                    a0 = words[cur + l] & c.rmask
                    ok, stride, dx = placement(c, blocked, a0, words[cur + l + 1], length)
                    if ok:
                        occ = mark(c, occ, a0, stride, dx, length)
                        cur += l + 2
                        placed = True
                        break
                l += 1
            if placed:
                break
            last_is_position = ((A & ~D) >> (nv - 1)) & 1
            if stats is not None:
                stats["windows_without_a_ship"] += 1
                stats["ended_on_a_position"] += int(last_is_position)
            cur += nv - 1 if last_is_position else nv
    return occ, cur


# ---- the oracle's boards ---------------------------------------------------------------------------------------------------------
def stream_matrix(t, stream):
    """[LANES][NWORDS] words of (SEED, LANE0 + i, t, stream), as Python ints"""
    nblk = NWORDS // 4
    ctr = np.zeros((LANES, nblk, 4), dtype=np.uint64)
    ctr[:, :, 0] = (LANE0 + np.arange(LANES, dtype=np.uint64))[:, None]
    ctr[:, :, 1] = t & 0xFFFFFFFF
    ctr[:, :, 2] = t >> 32
    ctr[:, :, 3] = (stream << 24) | np.arange(nblk, dtype=np.uint64)[None, :]
    key = np.array([SEED & 0xFFFFFFFF, SEED >> 32], dtype=np.uint64)
    return pr.philox4x32_10(ctr, key).reshape(LANES, NWORDS).tolist()


@pytest.fixture(scope="module")
def streams():
    return {"reset": stream_matrix(T0, pr.STREAM_RESET), "next0": stream_matrix(T0, pr.STREAM_NEXT),
            "next1": stream_matrix(T0 + 1, pr.STREAM_NEXT)}


def mask_ints(words):
    """uint32 [mw, n] -> one Python int per lane"""
    return [sum(int(words[j, i]) << (32 * j) for j in range(words.shape[0])) for i in range(words.shape[1])]


def oracle_boards(ol, size, max_len):
    """occ and next after batch_reset at T0, next after an episode end forced at T0 + 1 (which deals from stream NEXT of T0 + 1)"""
    from battleship_tapes import nearly_finished
    o = ol.OracleEnv("battleship", board_size=size, max_len=max_len)
    mw = mask_words(*size)
    st = o.new_state(LANES)
    o.batch_reset(st, SEED, LANE0, T0)
    occ, nxt = mask_ints(st[:mw]), mask_ints(st[2 * mw:])
    st, last = nearly_finished(st, size)
    _, rew, done, bad = o.batch_step(st, last, SEED, LANE0, T0 + 1)
    assert bad == 0 and done.all() and (rew == size[0] * size[1] - 1).all()
    assert mask_ints(st[:mw]) == nxt
    return occ, nxt, mask_ints(st[2 * mw:])


@pytest.mark.parametrize("size,max_len", BOARDS, ids=IDS)
def test_builders_equal_the_oracle(oracle_lib, streams, size, max_len):
    c = Consts(size[0], size[1], max_len)
    ships = sum(range(2, max_len + 1))
    stats = {"windows_without_a_ship": 0, "ended_on_a_position": 0}
    for name, want in zip(("reset", "next0", "next1"), oracle_boards(oracle_lib, size, max_len)):
        for i in range(LANES):
            words = streams[name][i]
            occ, used = board_sequential(c, words)
            ctx = (size, max_len, name, i)
            assert occ == want[i] and bin(occ).count("1") == ships and occ >> c.cells == 0, ctx
            assert board_feed(c, words) == (want[i], used), ctx
            assert board_feed2(c, words) == want[i], ctx
            assert board_windowed(c, words, stats) == (want[i], used), ctx


# ---- feed2 == feed; feed -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,max_len", BOARDS, ids=IDS)
def test_feed2_equals_two_feeds(streams, size, max_len):
    """from the states the boards of lanes 0 .. 3 pass through (every ship length left, both want_dir states, a0 over the board;
    every third one where rmask > 31), on every pair of word classes — a word acts through w & rmask alone (its low two bits
    are the direction) — where the board's rmask is at most 63, and on 3000 random pairs per state beyond"""
    c = Consts(size[0], size[1], max_len)
    rng = np.random.RandomState(c.cells * 16 + max_len)
    states = []
    for lane in range(4):
        b, i = Builder(c), 0
        while b.len >= 2:
            length = b.len
            feed(b, c, streams["next0"][lane][i])
            i += 1
            if b.len != length or i == 1:
                for want_dir in (False, True):
                    s = b.clone()
                    s.want_dir, s.a0 = want_dir, int(rng.randint(c.cells))
                    states.append(s)
    states.append(Builder(c))
    states = states[::1 if c.rmask <= 31 else 3]
    assert {(s.len, s.want_dir) for s in states} >= {(k, d) for k in range(2, max_len + 1) for d in (False, True)}
    if c.rmask <= 63:
        pairs = [(w0, w1) for w0 in range(c.rmask + 1) for w1 in range(c.rmask + 1)]
    else:
        pairs = [tuple(int(w) for w in p) for p in rng.randint(0, 1 << 32, (3000, 2), dtype=np.uint64)]
    for s in states:
        for w0, w1 in pairs:
            one, two = s.clone(), s.clone()
            feed(one, c, w0)
            feed(one, c, w1)
            feed2(two, c, w0, w1)
            assert one.live_key() == two.live_key(), (size, max_len, s.key(), w0, w1)


# ---- direction_words and the cursor ------------------------------------------------------------------------------------------
def test_direction_words_is_the_sequential_role_assignment():
    for off in (0, 1, 47, 48):
        for a16 in range(1 << 16):
            a = a16 << off
            assert direction_words(a) == sequential_roles(a), (off, a16)
    rng = np.random.RandomState(64)
    a = rng.randint(0, 1 << 32, 100000, dtype=np.uint64) | (rng.randint(0, 1 << 32, 100000, dtype=np.uint64) << np.uint64(32))
    a &= rng.randint(0, 1 << 32, 100000, dtype=np.uint64) | (rng.randint(0, 1 << 32, 100000, dtype=np.uint64) << np.uint64(32)) | \
        np.where(rng.rand(100000) < .5, np.uint64(2 ** 64 - 1), np.uint64(0))       # half of them dense, half with longer gaps
    d, prev_pos = np.zeros_like(a), np.zeros(len(a), bool)
    for l in range(64):                                                              # sequential_roles, all words at once
        bit = ((a >> np.uint64(l)) & np.uint64(1)).astype(bool)
        d |= prev_pos.astype(np.uint64) << np.uint64(l)
        prev_pos = ~prev_pos & bit
    even = np.uint64(0x5555555555555555)
    follows = a << np.uint64(1)
    got = (even ^ (((a & ~even & ~follows) + a) << np.uint64(1))) & follows
    assert np.array_equal(got, d)
    for x in a[:2000]:
        assert direction_words(int(x)) == sequential_roles(int(x))


@pytest.mark.parametrize("lead", [63, 61, 32])
def test_the_cursor_stops_before_an_accepted_position_at_the_windows_end(lead):
    """streams in which an acceptable position word is the last word of a window (word 63 of the first one): its direction
    word lies in the next window, so the cursor may only move up to it, not past it.  5x5, ships 3 and 2; 31 > 24 is a
    rejected position word; after the crafted words random ones, which the sequential parse reads the same way.
        63: 63 rejected words, then position 0 with direction N (cells 0, 5, 10)
        61: 61 rejected words, (24, N) leaves the board, then (0, N): a run of three acceptable words ends the window
        32: the first ship takes words 0 and 1, the cursor is at 2 — no refill — and the same window ends on position 2"""
    c = Consts(5, 5, 3)
    rng = np.random.RandomState(lead)
    tail = [int(w) for w in rng.randint(0, 1 << 32, 600, dtype=np.uint64)]
    if lead == 63:
        words = [31] * 63 + [0, 0] + tail
    elif lead == 61:
        words = [31] * 61 + [24, 0, 0, 0] + tail
    else:
        words = [0, 0] + [31] * 61 + [2, 0] + tail
    stats = {"windows_without_a_ship": 0, "ended_on_a_position": 0}
    occ, used = board_sequential(c, words)
    assert board_windowed(c, words, stats) == (occ, used)
    assert stats["ended_on_a_position"] >= 1
    if lead == 63:
        assert occ & 0b10000100001 == 0b10000100001


def test_windows_end_on_position_words_in_the_oracle_comparison_too(streams):
    """the board comparison above runs the cursor rule on real streams: on the narrow boards windows without a ship are common"""
    c = Consts(2, 13, 3)
    stats = {"windows_without_a_ship": 0, "ended_on_a_position": 0}
    for i in range(LANES):
        assert board_windowed(c, streams["next0"][i], stats) == board_sequential(c, streams["next0"][i])
    assert stats["ended_on_a_position"] > 0, stats


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X,Y", [(1, 16), (2, 13), (13, 2), (16, 7), (7, 16), (9, 10), (5, 5), (8, 8)])
def test_blocked_of_is_the_eight_neighbours_minus_nw(X, Y):
    """collision() looks at a cell and at Compass[0 .. 7] around it — N, E, S, W, NE, SE, SW; never at NW (-1, +1)"""
    c = Consts(X, Y, 2)
    rng = np.random.RandomState(X * 17 + Y)
    looks = [(0, 0), (0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1)]
    border_seen = 0
    for trial in range(300):
        density = (.03, .1, .3)[trial % 3]
        cells = [(x, y) for x in range(X) for y in range(Y) if rng.rand() < density]
        if trial < 2 * Y:                                                            # a lone cell in each border column
            cells = [((X - 1) * (trial & 1), trial >> 1)]
        occ = sum(1 << (y * X + x) for x, y in cells)
        border_seen += any(x in (0, X - 1) for x, _ in cells)
        want = 0
        for y in range(Y):
            for x in range(X):
                if any((x + dx, y + dy) in cells for dx, dy in looks):
                    want |= 1 << (y * X + x)
        got = blocked_of(occ, c)
        assert got & ((1 << c.cells) - 1) == want, (X, Y, cells)
    assert border_seen > 2 * Y


def test_wide_shifts_equal_plain_ones():
    rng = np.random.RandomState(128)
    for _ in range(2000):
        a = int(rng.randint(0, 1 << 32, dtype=np.uint64)) | int(rng.randint(0, 1 << 32, dtype=np.uint64)) << 32 | \
            int(rng.randint(0, 1 << 32, dtype=np.uint64)) << 64 | int(rng.randint(0, 1 << 32, dtype=np.uint64)) << 96
        for s in (1, 2, 15, 16, 17, 63):
            assert shl_small(a, s, 3) == (a << s) & (2 ** 128 - 1) and shr_small(a, s, 3) == a >> s


def test_the_division_by_multiplication_is_exact():
    for X in range(1, 17):
        inv_x = (65536 + X - 1) // X
        for a in range(128):
            assert (a * inv_x) >> 16 == a // X, (X, a)


def test_the_direction_constants_are_the_compass():
    for d in range(4):
        assert (sbfe(0xC4, 2 * d, 2), sbfe(0x31, 2 * d, 2)) == COMPASS[d]


def test_remaining_fits_its_six_bits():
    for max_len in range(2, 11):
        assert sum(range(2, max_len + 1)) < 64
    for (X, Y), _ in BOARDS:
        assert X * Y + 6 <= 32 * mask_words(X, Y) and (X * Y + 6 > 32 * (mask_words(X, Y) - 1))
    assert [mask_words(*b) for b, _ in BOARDS] == [1, 1, 1, 2, 3, 3, 3, 4, 4, 4, 4]
    assert 2 * 13 + 6 == 32 and 9 * 10 + 6 == 96 and 6 * 15 + 6 == 96           # the masks filled to the last bit
