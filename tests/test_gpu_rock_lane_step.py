"""RockSample's table-driven lane step (RockEnv<1, *>::step_rec, csrc/envs/rock.hip.h) in every loop that runs it, against the
CPU oracle: the rows of collect_synthetic, collect_tape and collect_returns over ~32 steps at the smallest batches at which the
launcher (csrc/fused_impl.hip.h: launch_steps_fused_l) still picks each loop —

    quad   a quad of lanes per thread: full 1024-lane workgroups from 3 * 2^18 lanes (StochasticRock: 2^19);
    half   half a quad per thread: above 3 * 2^17 lanes (StochasticRock: from 3 * 2^17), 4-byte sinks only — the returns sink
           has no such loop, so that launch is left out of this case;
    lane   one lane per thread, the small shards' loop: full 256-lane workgroups (RockSample only) — more than one workgroup,
           and as many lanes as it takes for the oracle's rows to hold every outcome (an exit to the east is rare).

The boards: RockSample(7,8); RockSample(11,11), the largest board with one state word that the reference configures (rock.py:43-64
lists 1, 3, 7 / 8, 11 and 15 rocks) and the oracle builds — its last rock's code lies at bits 28-29; RockSample(2,1), the smallest
table; StochasticRock(7,8), whose penalties neither cost nor end anything.  Twelve rocks — the most one state word holds, the
last code at bits 30-31 — exist in no reference configuration, so no oracle row can speak for them: the last test gives
RockSample(15, .) twelve rocks through the parameter block and holds the table-driven loops to the arithmetic lane step
(RockEnv::step_pre, which launches shorter than 16 steps take), on a tape that walks every lane onto that rock.

What keeps the comparison honest is asserted from the ORACLE's rows, not the kernel's: every action, every outcome (-10, -100
and done, +10 for a sample, +10 and done for the exit, 0), both readings of a CHECK, a SAMPLE on an empty cell, on a collected
rock and on a live one, and an auto-reset in each of a quad's four lane positions."""
import numpy as np
import pytest
import torch

from test_gpu_parity import make_env, np_

pytestmark = pytest.mark.gpu

STEPS = 32
BOARDS = {"rock-7-8": ("rock", {}), "rock-11-11": ("rock", dict(board_size=11, num_rocks=11)),
          "rock-2-1": ("rock", dict(board_size=2, num_rocks=1)), "stochrock-7-8": ("stochrock", {})}
# loop -> (lanes, what pomdp_last_fused_kernel() ends with besides the sink)
ROCK_LOOPS = {"quad": 3 << 18, "half": (3 << 17) + 4096, "lane": 1 << 15}
STOCH_LOOPS = {"quad": 1 << 19, "half": 3 << 17}
CASES = [(b, l, n) for b in BOARDS for l, n in (STOCH_LOOPS if b.startswith("stoch") else ROCK_LOOPS).items()]


def kernel_name(board, loop, sink):
    env = "StochasticRockEnv<1>" if board.startswith("stoch") else "RockEnv<1>"
    if loop == "lane":
        return "steps_kernel<%s, 1, true, true, %s>" % (env, sink)
    return "steps_quad_kernel<%s, %s%s>" % (env, sink, ", 2" if loop == "half" else "")


class Seen(object):
    """what the oracle's rows of a run held (see the module's docstring)"""

    def __init__(self, env, kw, n_actions):
        from gym_pomdp_amd import tables
        self.stoch, self.n_actions = env == "stochrock", n_actions
        rocks = tables.ROCK_CONFIG[kw.get("board_size", 7)][2][:kw.get("num_rocks", 8)]
        self.grid = np.full(256, -1, np.int64)
        for j, (x, y) in enumerate(rocks):
            self.grid[x | y << 4] = j
        self.flags = set()

    def row(self, pre, a, ob, rew, done):
        pre, a, done = pre.astype(np.int64), a.astype(np.int64), done.astype(bool)
        rid = self.grid[pre & 0xFF]
        code = (pre >> (8 + 2 * np.maximum(rid, 0))) & 3
        f = self.flags
        f.update(("action", int(v)) for v in np.unique(a[a < self.n_actions]))
        for name, m in (("-10", rew == -10), ("-100 and done", (rew == -100) & done), ("+10 sample", (rew == 10) & (a == 4) & ~done),
                        ("+10 exit and done", (rew == 10) & (a == 1) & done), ("0", (rew == 0) & (a < self.n_actions)),
                        ("check ob 1", (a >= 5) & (a < self.n_actions) & (ob == 1)), ("check ob 2", (a >= 5) & (a < self.n_actions) & (ob == 2)),
                        ("sample empty", (a == 4) & (rid < 0)), ("sample collected", (a == 4) & (rid >= 0) & (code == 1)),
                        ("sample live", (a == 4) & (rid >= 0) & (code != 1))):
            if m.any():
                f.add(name)
        f.update(("reset in lane", int(v)) for v in np.unique(np.nonzero(done)[0] & 3))

    def missing(self, exit_reachable=True):
        want = {("action", v) for v in range(self.n_actions)} | {("reset in lane", v) for v in range(4)} | {
            "-10", "+10 sample", "+10 exit and done", "0", "check ob 1", "check ob 2", "sample empty", "sample collected", "sample live"}
        if not self.stoch:
            want.add("-100 and done")          # StochasticRock's penalty is 0 and ends nothing (rock.py:432, 503)
        if not exit_reachable:
            want.discard("+10 exit and done")
        return sorted(map(str, want - self.flags))


def oracle_rows(oracle_lib, o, seen, st, seed, lane0, t0, steps, tape=None):
    """steps of the oracle from `st` (advanced in place) under the synthetic policy or a tape -> [(action, ob, reward, done)], bad"""
    nt, n = oracle_lib.max_threads(), st.shape[1]
    rows, done, n_bad = [], np.zeros(n, np.uint8), 0
    for k in range(steps):
        t = t0 + 1 + k
        a = tape[k].astype(np.int32) if tape is not None else oracle_lib.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt)
        pre = st[0].copy()
        ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
        n_bad += bad
        seen.row(pre, a, ob, rew, done)
        rows.append((a, ob, rew, done.astype(bool)))
    return rows, n_bad


def tape_of(n_actions, steps, n, size=0):
    """uniform actions no policy of ours drew, one byte in 4096 out of range; every eighth lane first walks east off a board of
    `size` columns (the exit: eleven moves east in a row are beyond a uniform policy's 32 steps)"""
    rng = np.random.RandomState(n % 9973 + steps)
    tape = rng.randint(0, n_actions, (steps, n)).astype(np.uint8)
    bad = rng.randint(0, 4096, (steps, n)) == 0
    tape[bad] = rng.randint(n_actions, 256, int(bad.sum())).astype(np.uint8)
    tape[:size, ::8] = 1
    return tape


@pytest.mark.parametrize("board,loop,n", CASES, ids=["%s-%s" % c[:2] for c in CASES])
def test_lane_step_rows_equal_the_oracle(oracle_lib, board, loop, n):
    from gym_pomdp_amd import EpisodeStats, _native
    L = _native.lib()
    env, kw = BOARDS[board]
    seed, lane0, t0 = 20261018, 1 << 20, (1 << 32) + 3
    nt = oracle_lib.max_threads()
    o = oracle_lib.OracleEnv(env, **kw)

    def fresh():
        e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
        e.call_counter = t0
        st = o.new_state(n)
        assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, t0, nthreads=nt))
        return e, st

    def compare(cols, rows, ctx, with_action=True):
        for k, (a, ob, rew, done) in enumerate(rows):
            if with_action:
                assert np.array_equal(np_(cols["action"][k]), a), ctx + (k,)
            assert np.array_equal(np_(cols["ob"][k]), ob), ctx + (k,)
            assert np.array_equal(np_(cols["reward"][k]), rew), ctx + (k,)
            assert np.array_equal(np_(cols["done"][k]), done), ctx + (k,)

    # the synthetic policy, packed records
    e, st = fresh()
    seen = Seen(env, kw, o.n_actions)
    rows, bad = oracle_rows(oracle_lib, o, seen, st, seed, lane0, t0, STEPS)
    # (RockSample(11,11): no lane of the synthetic policy gets eleven columns east in 32 steps; the tape below walks there)
    assert bad == 0 and seen.missing(kw.get("board_size", 7) < 11) == [], (board, loop, "synthetic", seen.missing())
    cols = e.decode_trajectory(e.collect_synthetic(STEPS, layout="packed"), STEPS)
    assert L.pomdp_last_fused_kernel().decode() == kernel_name(board, loop, "Packed"), L.pomdp_last_fused_kernel()
    compare(cols, rows, (board, loop, "synthetic"))
    assert np.array_equal(np_(e.state).view(np.uint32), st) and e.invalid_action_count() == 0
    want_state = st

    # the returns sink over the same steps (no half-quad form)
    if loop != "half":
        e, st = fresh()
        stats = EpisodeStats(e)
        acc, cnt = oracle_lib.new_return_stats(n)
        o.batch_collect_returns(st, acc, cnt, e._discount, seed, lane0, t0 + 1, STEPS, nthreads=nt)
        assert np.array_equal(st, want_state)
        e.collect_returns(STEPS, stats)
        assert L.pomdp_last_fused_kernel().decode() == kernel_name(board, loop, "Returns"), L.pomdp_last_fused_kernel()
        for q, name in enumerate(("ret", "disc", "ret_done", "ret_sum")):
            assert np.array_equal(np_(getattr(stats, name)).view(np.uint64), acc[q].view(np.uint64)), (board, loop, name)
        assert np.array_equal(np_(stats.episodes), cnt[0]) and np.array_equal(np_(stats.steps), cnt[1])
        assert np.array_equal(np_(e.state).view(np.uint32), st)

    # the caller's tape, packed records
    e, st = fresh()
    seen = Seen(env, kw, o.n_actions)
    tape = tape_of(o.n_actions, STEPS, n, kw.get("board_size", 7))
    rows, bad = oracle_rows(oracle_lib, o, seen, st, seed, lane0, t0, STEPS, tape)
    assert bad == int((tape >= o.n_actions).sum()) > 0 and seen.missing() == [], (board, loop, "tape", seen.missing())
    cols = e.decode_trajectory(e.collect_tape(torch.as_tensor(tape, device="cuda"), layout="packed"), STEPS)
    assert L.pomdp_last_fused_kernel().decode() == kernel_name(board, loop, "Packed, Tape"), L.pomdp_last_fused_kernel()
    compare(cols, rows, (board, loop, "tape"))
    assert np.array_equal(np_(e.state).view(np.uint32), st) and e.invalid_action_count() == bad


def test_twelve_rocks_table_step_equals_the_arithmetic_step(monkeypatch):
    """K = 12: rock 11's code lies at bits 30-31 of the state word, where collecting a good rock is a step of -1 << 30.  Every lane
    walks to that rock at (9, 1), CHECKs it (from distance 0 the reading is the rock's own code), samples it (+10 or -10 by the
    lane's own reset draw), samples it again (collected:
    -100 and done), then follows a random tape.  One launch of 32 steps (the table) against four of 8 (the arithmetic step)."""
    from gym_pomdp_amd import _native, tables
    L = _native.lib()
    sizes, start, rocks = tables.ROCK_CONFIG[15]
    assert start == (0, 5) and rocks[11] == (9, 1) and rocks.index((9, 1)) == 11
    monkeypatch.setitem(tables.ROCK_CONFIG, 15, (tuple(sizes) + (12,), start, rocks))
    kw, seed, lane0, t0 = dict(board_size=15, num_rocks=12), 20261018, 1 << 20, (1 << 32) + 3
    walk = [1] * 9 + [2] * 4 + [16, 4, 4]
    for loop, n in ROCK_LOOPS.items():
        tape = tape_of(17, STEPS, n)
        tape[:len(walk)] = np.asarray(walk, np.uint8)[:, None]
        d_tape = torch.as_tensor(tape, device="cuda")
        got = {}
        for fuse in (_native.FUSE_MAX_DEFAULT, 8):
            L.pomdp_fuse_max(fuse)
            try:
                e = make_env("rock", kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
                e.call_counter = t0
                e.reset()
                cols = e.decode_trajectory(e.collect_tape(d_tape, layout="packed"), STEPS)
                name = L.pomdp_last_fused_kernel().decode()
            finally:
                L.pomdp_fuse_max(_native.FUSE_MAX_DEFAULT)
            got[fuse] = {k: np_(v[:STEPS]).astype(np.int64) for k, v in cols.items()}, np_(e.state).view(np.uint32), e.invalid_action_count(), name
        (tab, tab_state, tab_bad, tab_name), (ari, ari_state, ari_bad, ari_name) = got[_native.FUSE_MAX_DEFAULT], got[8]
        assert tab_name == kernel_name("rock", loop, "Packed, Tape"), tab_name
        assert ari_name == "steps_kernel<RockEnv<1>, 1, true, false, Packed, Tape>", ari_name
        # the arithmetic step's rows hold what the walk is for: both codes of rock 11 sampled, both readings, the second SAMPLE's penalty
        r = ari["reward"]
        assert set(np.unique(ari["ob"][13])) == {1, 2} and set(np.unique(r[14])) == {-10, 10} and (r[15] == -100).all() and ari["done"][15].all()
        for k in tab:
            assert np.array_equal(tab[k], ari[k]), (loop, k)
        assert np.array_equal(tab_state, ari_state) and tab_bad == ari_bad > 0
