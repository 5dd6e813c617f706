"""CPU restatement of the bounded History's window (include/pomdp_hip.h: pomdp_history; csrc/planner.hip: history_push,
history_append_kernel, history_clear_kernel), in numpy: the two per-rock sums as a walk over the oracle's records
(window_sums), the ring's bytes back as records (decode_ring), the ring contract itself (Ring) and the transition streams
test_history_window_host.py and test_gpu_history_window.py both run (stream).  None of it reads the HIP side's arrays to
decide what is right: the records are oracle_lib.HistorySums.rec, kept as the reference keeps them (rock.py:533-544)."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
SEED = 20261018
GARBAGE_NEXT = (3, 4, 5, -1)
# the (K, max_size) grid of the GPU test, with the RockSample configuration that has K rocks; Python's make_params takes
# num_rocks from tables.ROCK_CONFIG, whose largest is 15 (the C side allows 16), so bit 15 + 16 = 31 of move_ok is not reached
ROCK_KW = {1: dict(board_size=2, num_rocks=1), 8: dict(board_size=7, num_rocks=8), 15: dict(board_size=15, num_rocks=15)}
MAX_SIZES = (0, 1, 2, 3, 63, 255)
N_LANES = 515                                   # not a multiple of the workgroup size, and n % 4 != 0


def garbage_actions(K):
    """& 31 sends 37, 69 and -27 to CHECK 0 and 38 to CHECK 1; 5 + K is the first CHECK this env does not have"""
    return (37, 38, 69, -27, -1, 5 + K, 1 << 20, INT32_MIN)


def n_appends(max_size):
    return 3 * (max_size + 1) + 40              # the ring wraps at least twice on a lane that is never reset


def window_sums(hs, K):
    """(total_sample, total_move) int32 [K, n] of the records a bounded oracle_lib.HistorySums holds — history_total of
    oracle/pomdp_oracle.c, i.e. rock.py:303-310 and 327-334: over the records with action == j + 5,
    sample = #(next == 2) - #(next == 1), move = #(next == 2) - #(next != 2 and observation == 1)."""
    obs, act, nxt = hs.rec
    rows, n = act.shape
    ts, tm = np.zeros((K, n), np.int32), np.zeros((K, n), np.int32)
    if K == 0 or rows == 0:
        return ts, tm
    r, lane = np.nonzero((np.arange(rows)[:, None] < hs.size[None, :]) & (act >= 5) & (act < 5 + K))
    cell = (act[r, lane].astype(np.int64) - 5) * n + lane
    good, bad = nxt[r, lane] == 2, nxt[r, lane] == 1
    neg = ~good & (obs[r, lane] == 1)
    add = lambda w: np.bincount(cell, weights=w, minlength=K * n).reshape(K, n)       # noqa: E731  (small integers: exact)
    ts[:] = add(good.astype(np.float64) - bad)
    tm[:] = add(good.astype(np.float64) - neg)
    return ts, tm


def move_ok_word(ts, tm):
    """pomdp_history.move_ok: bit j = total_move[j] >= 0, bit 16 + j = total_sample[j] > 0 -> int64 [n]"""
    w = (1 << np.arange(ts.shape[0], dtype=np.int64))[:, None]
    return ((tm >= 0) * w).sum(axis=0) | (((ts > 0) * w).sum(axis=0) << 16)


def decode_ring(ring, head, size, W):
    """The window a ring of W rows holds, oldest first -> dict(action, next, bad, valid), each [W, n]: rows (head + r) % W
    once size == W and rows 0 .. size - 1 before that; a byte is action | next_ob << 5 | (observation == BAD) << 7."""
    ring = np.asarray(ring, np.uint8).reshape(W, -1)
    r = np.arange(W)[:, None]
    idx = np.where(size[None, :] == W, (head[None, :].astype(np.int64) + r) % W, r)
    b = np.take_along_axis(ring, idx, axis=0).astype(np.int32)
    return dict(action=b & 31, next=(b >> 5) & 3, bad=b >> 7, valid=r < size[None, :])


def canonical(K, obs, act, nxt):
    """what a record of the window must read as, whatever int32 the caller appended: the CHECK's rock (-1: not a CHECK of
    this env), next == GOOD, next == BAD, observation == BAD — the four things the two sums take from a record"""
    chk = np.where((act >= 5) & (act < 5 + K), act - 5, -1)
    return chk, nxt == 2, nxt == 1, obs == 1


class Ring(object):
    """The ring contract, lane-parallel: push (with the eviction of the oldest record once max_size + 1 are kept), clear and
    the auto-reset on a terminal transition.  A record enters the sums with what `canonical` says of it and leaves with
    exactly that: an action that is no CHECK of this env is kept as a non-CHECK (an out-of-range one as 31), a next
    observation outside 1..2 as 0.  `mutant` names one deliberate departure (test_history_window_host.py lists them)."""
    MUTANTS = ("no_subtract", "evict_newest", "short_window", "head_kept", "bit7_dropped", "sums_kept", "raw_byte")

    def __init__(self, K, n, max_size, mutant=None):
        assert mutant is None or mutant in self.MUTANTS
        self.K, self.n, self.mutant = K, n, mutant
        self.W = max(max_size, 1) if mutant == "short_window" else max_size + 1
        self.ring = np.zeros((self.W if K else 0, n), np.uint8)
        self.head, self.size = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.last_action, self.last_ob = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        self.total_sample, self.total_move = np.zeros((K, n), np.int32), np.zeros((K, n), np.int32)

    def clear(self, where=None):
        w = np.ones(self.n, bool) if where is None else np.asarray(where) != 0
        self.size[w] = 0; self.last_action[w] = -1; self.last_ob[w] = -1
        if self.mutant != "head_kept":
            self.head[w] = 0
        self.total_sample[:, w] = 0; self.total_move[:, w] = 0

    def _add(self, lanes, byte, sign):
        a, nx, bad = byte & 31, (byte >> 5) & 3, byte >> 7
        if sign < 0 and self.mutant == "bit7_dropped":
            bad = np.zeros_like(bad)
        m = (a >= 5) & (a < 5 + self.K)
        cell = (a[m] - 5).astype(np.int64) * self.n + lanes[m]
        cnt = lambda w: np.bincount(cell, weights=w, minlength=self.K * self.n).reshape(self.K, self.n).astype(np.int32)   # noqa: E731
        self.total_sample += sign * cnt((nx[m] == 2).astype(np.float64) - (nx[m] == 1))
        self.total_move += sign * cnt(np.where(nx[m] == 2, 1., -(bad[m] != 0).astype(np.float64)))

    def append(self, obs, act, nxt, done, auto_reset):
        obs, act, nxt = (np.asarray(v, np.int32) for v in (obs, act, nxt))
        fresh = (np.asarray(done) != 0) & bool(auto_reset)
        if self.mutant == "sums_kept":
            ts, tm = self.total_sample.copy(), self.total_move.copy()
            self.clear(fresh)
            self.total_sample, self.total_move = ts, tm
        else:
            self.clear(fresh)
        lanes = np.nonzero(~fresh)[0]
        o, a, x = obs[lanes], act[lanes].astype(np.int64), nxt[lanes].astype(np.int64)
        if self.mutant == "raw_byte":                                  # the byte of whatever came in, unmasked
            byte = ((a | (x << 5) | ((o == 1) * 128)) & 255).astype(np.int32)
            chk, good, badn, pbad = canonical(self.K, o, a, x)
            enter = (np.where(chk >= 0, chk + 5, 0) | (good * 2 + badn * 1) << 5 | pbad * 128).astype(np.int32)
        else:
            ca = np.where((a >= 0) & (a < 5 + self.K), a, 31)
            cx = np.where((x == 1) | (x == 2), x, 0)
            byte = enter = (ca | (cx << 5) | ((o == 1) * 128)).astype(np.int32)
        if self.K:
            full = self.size[lanes] == self.W
            slot = self.head[lanes].copy()
            if self.mutant == "evict_newest":
                slot = np.where(full, (slot + self.W - 1) % self.W, slot)
            if self.mutant != "no_subtract":
                self._add(lanes[full], self.ring[slot[full], lanes[full]].astype(np.int32), -1)
            self.ring[slot, lanes] = byte
            if self.mutant == "evict_newest":
                self.head[lanes] = np.where(full, self.head[lanes], (self.head[lanes] + 1) % self.W)
            else:
                self.head[lanes] = (self.head[lanes] + 1) % self.W
            self._add(lanes, enter, 1)
        self.size[lanes] = np.minimum(self.size[lanes] + 1, self.W)
        self.last_action[lanes] = act[lanes]; self.last_ob[lanes] = nxt[lanes]

    def window(self):
        return decode_ring(self.ring, self.head, self.size, self.W)


def stream(K, n, steps, garbage=False, seed=SEED):
    """The transitions both tests append: a list of (observation, action, next_observation, done, auto_reset) per step,
    int32 [n] / uint8 [n] / bool.  Well over half of the actions are CHECKs of two or three `hot` rocks (different ones per
    lane), so that a window holds dozens of records of one rock and the sums run far from 0; the rest are moves, SAMPLE and
    a CHECK of every other rock.  next_ob is drawn from {0, 1, 1, 2, 2}, observation from {0, 1, 1, 2}.  `done` comes with
    probability 1 / 40 over the batch: never on the lanes with i % 8 < 3 — whose ring therefore fills and wraps whatever the
    window's length — and with probability 1 / 25 on the others.  auto_reset is off every third step, so terminal records
    are appended too.  With `garbage`, one action in six is one of garbage_actions(K) and one next observation in six one
    of GARBAGE_NEXT: values History.append() accepts (any int32) that no env produces."""
    rng = np.random.default_rng([seed, K, n, steps, int(garbage)])
    lane = np.arange(n)
    n_hot = min(K, 3)
    hot = (lane[:, None] + np.arange(max(n_hot, 1))[None, :] * 2) % max(K, 1)          # [n, n_hot]
    out = []
    for t in range(steps):
        u = rng.random(n)
        act = rng.integers(0, 5, n)                                                   # moves and SAMPLE
        if K:
            act = np.where(u < .10, 5 + rng.integers(0, K, n), act)                   # a CHECK of any rock
            act = np.where(u >= .35, 5 + hot[lane, rng.integers(0, n_hot, n)], act)   # 65 %: a CHECK of a hot rock
        nxt = rng.choice(np.array([0, 1, 1, 2, 2]), n)
        obs = rng.choice(np.array([0, 1, 1, 2]), n)
        done = (rng.random(n) < 1. / 25) & (lane % 8 >= 3)
        if garbage:
            g = rng.random(n) < 1. / 6
            act = np.where(g, rng.choice(np.array(garbage_actions(K), np.int64), n), act)
            g = rng.random(n) < 1. / 6
            nxt = np.where(g, rng.choice(np.array(GARBAGE_NEXT), n), nxt)
        out.append((obs.astype(np.int32), act.astype(np.int32), nxt.astype(np.int32), done.astype(np.uint8), t % 3 != 2))
    return out


def clear_masks(n, max_size, seed=SEED):
    """{step: where}: clear() on a random third of the lanes before that step's append — once while the window is still
    filling and once after max_size + 1 appends and more, when the never-reset lanes' rings are full"""
    rng = np.random.default_rng([seed, n, max_size, 7])
    W = max_size + 1
    return {W // 2 + 3: (rng.random(n) < 1. / 3).astype(np.uint8), W + 20: (rng.random(n) < 1. / 3).astype(np.uint8)}
