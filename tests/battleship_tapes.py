"""BattleShip action tapes that end episodes on purpose, and nearly finished states (a helper: no tests in here).

Under a uniform policy a 10x10 board takes about 325 steps, so a 64-step launch of the fused loops sees almost no episode end
on any board larger than 5x5.  The tapes here are built WHILE the CPU oracle steps (before any GPU work): unless its schedule
says otherwise, lane i's byte at a step is the lowest set bit of occ & ~vis of the oracle's current state of that lane — a sure
hit — so an episode lasts exactly S = 2 + 3 + .. + max_len steps.

    volley        no deviation: every lane ends at steps S - 1, 2 S - 1, ..; a wave queues all its lanes at once, and from the
                  second end of a launch on the builder pool runs in the middle of the loop (`again`) for the whole wave
    stagger(P)    at the start of each episode lane i first shoots (i mod P) times at its lowest unvisited EMPTY cell (a miss,
                  reward -1): with P > S some lane ends an episode at every step from S - 1 on
    revisit       one lane-step in about 50 shoots at the lane's lowest visited cell instead (reward -10, nothing changes)
    bad           one lane-step in about 1000 gets a byte outside the action range (n_actions .. 255): the lane is untouched
Every byte is chosen from the oracle's state first and the oracle stepped with it afterwards, so a revisit or an out-of-range
byte just shifts the lane's plan by a step.

The coverage counts come from the oracle's `done` rows and the launch cuts, never from the GPU:
    ends          episode ends in the collection
    again         (lane, launch) pairs with two or more ends: the second one finds the lane's next board still unbuilt
    max_pending   the largest number of lanes of one wave (64 * LPT consecutive lanes) waiting at one build; a wave builds when
                  one of its waiting lanes ends again, and when the launch ends
"""
import numpy as np


def ship_cells(max_len):
    return sum(range(2, max_len + 1))


def mask_words(size):
    return (size[0] * size[1] + 6 + 31) // 32


def _valid_words(size):
    """uint32 [MW, 1]: the bits of each mask word that are cells of the board"""
    cells, mw = size[0] * size[1], mask_words(size)
    return np.array([[(1 << min(max(cells - 32 * j, 0), 32)) - 1] for j in range(mw)], dtype=np.uint64).astype(np.uint32)


def lowest_bit(words):
    """index of the lowest set bit of each lane's mask (uint32 [MW, n]); -1 where the mask is empty"""
    out = np.full(words.shape[1], -1, np.int64)
    for j in range(words.shape[0] - 1, -1, -1):
        w = words[j].astype(np.int64)
        low = w & -w
        idx = np.log2(np.maximum(low, 1)).astype(np.int64)                 # exact: a power of two
        out = np.where(w != 0, 32 * j + idx, out)
    return out


def masks(st, size):
    """(occ, vis, unvisited ships, unvisited empty cells) as uint32 [MW, n] of a packed state"""
    mw = mask_words(size)
    valid = _valid_words(size)
    occ, vis = st[:mw], st[mw:2 * mw].copy()
    vis[mw - 1] &= np.uint32(0x03FFFFFF)
    return occ, vis, occ & ~vis, ~occ & ~vis & valid


def nearly_finished(st, size):
    """From a packed state: every cell visited except one ship cell per lane (lane i keeps its (i mod ships)-th ship cell),
    remaining = 1.  occ and next are kept.  -> (state, the action that ends each lane's episode)"""
    mw = mask_words(size)
    valid = _valid_words(size)
    st = st.copy()
    n = st.shape[1]
    left = st[:mw].copy()
    ships = sum(np.unpackbits(left[j].view(np.uint8)).reshape(n, 32).sum(axis=1) for j in range(mw))
    assert (ships == ships[0]).all()
    drop = np.arange(n) % int(ships[0])                                    # clear that many of the lowest ship cells first
    for k in range(int(ships[0])):
        a = lowest_bit(left)
        hit = (drop > k)
        for j in range(mw):
            bit = np.where(hit & (a >> 5 == j), np.uint32(1) << (a & 31).astype(np.uint32), np.uint32(0)).astype(np.uint32)
            left[j] &= ~bit
    last = lowest_bit(left)
    for j in range(mw):
        bit = np.where(last >> 5 == j, np.uint32(1) << (last & 31).astype(np.uint32), np.uint32(0)).astype(np.uint32)
        st[mw + j] = valid[j] & ~bit
    st[2 * mw - 1] |= np.uint32(1 << 26)
    return st, last.astype(np.int32)


def coverage(done, cuts, lpt):
    """done: bool [steps, n]; cuts: the launch lengths in order; lpt: lanes per thread (a wave is 64 * lpt lanes)"""
    steps, n = done.shape
    wave = 64 * lpt
    assert sum(cuts) == steps and n % wave == 0
    again, max_pending, s = 0, 0, 0
    for k in cuts:
        seg = done[s:s + k]
        again += int((seg.sum(axis=0) >= 2).sum())
        pend = np.zeros(n, bool)
        for row in seg:
            fire = (row & pend).reshape(-1, wave).any(axis=1)               # a waiting lane of the wave ends again: build now
            counts = pend.reshape(-1, wave).sum(axis=1)
            if fire.any():
                max_pending = max(max_pending, int(counts[fire].max()))
                pend &= ~np.repeat(fire, wave)
            pend |= row
        max_pending = max(max_pending, int(pend.reshape(-1, wave).sum(axis=1).max()))
        s += k
    return {"ends": int(done.sum()), "again": again, "max_pending": max_pending}


def launch_cuts(steps, fuse):
    return [fuse] * (steps // fuse) + ([steps % fuse] if steps % fuse else [])


class Tape(object):
    """The oracle's trajectory from reset() at t0 on a tape built along the way.  `pre` steps come first (tape_pre; the state
    after them is st_pre): the collection that is compared — `steps` rows, from call counter t0 + 1 + pre — can then begin
    where episodes already end.  Attributes as test_gpu_key_edges.Ref has them (action, ob, reward, done, st, bad, ..), so
    Ref.check_cols and Ref.returns work on it."""

    def __init__(self, ol, size, max_len, n, steps, seed, lane0, t0, schedule="volley", period=0, revisit=False, bad=False, pre=0,
                 tape_seed=1):
        kw = self.kw = dict(board_size=size, max_len=max_len)
        self.ol, self.o, self.n, self.steps, self.pre = ol, ol.OracleEnv("battleship", **kw), n, steps, pre
        self.seed, self.lane0, self.t_reset, self.t0 = seed, lane0, t0, t0 + pre
        assert schedule in ("volley", "stagger") and (schedule == "volley") == (period == 0)
        o, nt = self.o, ol.max_threads()
        self.nt = nt
        st = o.new_state(n)
        self.ob_reset = o.batch_reset(st, seed, lane0, t0, nthreads=nt)
        self.st_reset = st.copy()
        rng = np.random.RandomState(tape_seed)
        n_act = o.n_actions
        plan = (np.arange(n) % period) if period else np.zeros(n, np.int64)
        misses = plan.copy()
        done = np.zeros(n, np.uint8)
        tape = np.zeros((pre + steps, n), np.uint8)
        rows, self.bad = [], 0
        for k in range(pre + steps):
            if k == pre:
                self.st0 = st.copy()
            occ, vis, ships_left, empty_left = masks(st, size)
            hit, miss = lowest_bit(ships_left), lowest_bit(empty_left)
            assert (hit >= 0).all() and (miss[misses > 0] >= 0).all()
            a = np.where(misses > 0, miss, hit)
            planned = np.ones(n, bool)
            if revisit:
                seen = lowest_bit(vis)
                again = (rng.randint(0, 50, n) == 0) & (seen >= 0)
                a, planned = np.where(again, seen, a), planned & ~again
            if bad:
                out = rng.randint(0, 1000, n) == 0
                a, planned = np.where(out, rng.randint(n_act, 256, n), a), planned & ~out
            tape[k] = a
            a32 = a.astype(np.int32)
            ob, rew, done, nbad = o.batch_step(st, a32, seed, lane0, t0 + 1 + k, auto_reset=True, done=done, nthreads=nt)
            misses = np.where(done != 0, plan, misses - (planned & (misses > 0)))
            if k >= pre:
                self.bad += nbad
                rows.append((a32, ob, rew, done.copy()))
        self.tape_pre, self.tape = tape[:pre], tape[pre:]
        self.st = st
        self.action, self.ob, self.reward, self.done = (np.stack([r[i] for r in rows]) for i in range(4))

    def coverage(self, fuse, lpt):
        return coverage(self.done.astype(bool), launch_cuts(self.steps, fuse), lpt)

    def returns(self, discount, pitch):
        """or_batch_collect_returns fed the same tape from the same state: (acc, cnt)"""
        st = self.st0.copy()
        acc, cnt = self.ol.new_return_stats(self.n, pitch)
        self.o.batch_collect_returns(st, acc, cnt, discount, self.seed, self.lane0, self.t0 + 1, self.steps, nthreads=self.nt,
                                     actions=self.tape.astype(np.int32))
        assert np.array_equal(st, self.st)
        return acc, cnt
