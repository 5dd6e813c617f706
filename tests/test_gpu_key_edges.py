"""Every launch that draws random words, at the edges of the Philox key and counter.  The other GPU tests keep the seed below
2^32 (key word k1 == 0), the call counter's high word at 0 .. 2 and the lanes far below 2^32; the timed kernels no longer call
philox4x32_10 but hand-specialised forms of it (philox_fixed, SyntheticQuad's own key copies, cx.key's carried counter, the
board builders' counter), so a dropped k1 or a lost carry would pass there.  Here every comparison is with the CPU oracle
(pinned to the reference at these coordinates by tests/test_reference_live.py and to oracle/philox_ref.py by
tests/test_oracle_golden.py), bit for bit: int rows, uint32 state words, float64 returns viewed as uint64.

    K1  seed 0x9E3779B97F4A7C15, the last quad of the batch is the top one (lane0 = 2^32 - n, n rounded up to 4), reset at
        t = 2^32 - 7: the env's call counter carries into its high word at the sixth step, the policy's one step earlier
    K2  seed 2^32 (k0 = 0, k1 = 1), lane0 = 2^22, reset at t = 0xFFFFFFFE_FFFFFFF9: t_hi carries to 0xFFFFFFFF mid-launch
    K3  seed 2^64 - 1, lane0 = 0, t = 0
K1 runs on every row, K2 and K3 on the quad-gate row of each env and sink and on the planner's.  Sizes are the launcher's
gates (test_launcher_picks_the_documented_kernel_per_shard_size) and 20 steps in one launch (8 where RockSample's arithmetic
step or Tag's table-free loop is meant)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import make_env, np_
from test_gpu_timed_kernels import _heuristic_fused_vs_oracle, _tape, fuse64  # noqa: F401  (fuse64: a fixture)
from test_gpu_episodes import Pair, check_returns, check_rows, random_tape

pytestmark = pytest.mark.gpu

KS = ("K1", "K2", "K3")
ROCK15 = dict(board_size=15, num_rocks=15)
NET16 = dict(n_machines=16, problem_type=1)


def coords(K, n):
    """(seed, lane0, t0) of a coordinate set for a batch of n lanes; lane0 is a multiple of 4"""
    if K == "K1":
        return 0x9E3779B97F4A7C15, (1 << 32) - (n + 3) // 4 * 4, (1 << 32) - 7
    if K == "K2":
        return 1 << 32, 1 << 22, 0xFFFFFFFEFFFFFFF9
    return (1 << 64) - 1, 0, 0


def last_kernel():
    from gym_pomdp_amd import _native
    return _native.lib().pomdp_last_fused_kernel().decode()


def kwid(kw):
    return "-".join(str(v) for v in kw.values())


class Ref(object):
    """The oracle's trajectory of `steps` auto-resetting steps from reset() at t0, under the synthetic policy of `pol_seed` or on
    a tape: computed once, compared with every sink."""

    def __init__(self, ol, env, kw, n, steps, seed, lane0, t0, tape=None, pol_seed=None):
        self.ol, self.o, self.n, self.steps = ol, ol.OracleEnv(env, **kw), n, steps
        self.seed, self.lane0, self.t0, self.tape = seed, lane0, t0, tape
        nt = self.nt = ol.max_threads()
        o, st = self.o, None
        st = self.st = o.new_state(n)
        self.ob0 = o.batch_reset(st, seed, lane0, t0, nthreads=nt)
        self.st0 = st.copy()
        ps = seed if pol_seed is None else pol_seed
        done = np.zeros(n, np.uint8)
        rows, self.bad = [], 0
        for k in range(steps):
            t = t0 + 1 + k
            a = ol.synthetic_actions(n, ps, lane0, t, o.n_actions, nthreads=nt) if tape is None else tape[k].astype(np.int32)
            ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
            self.bad += bad
            rows.append((a, ob, rew, done.copy()))
        self.action, self.ob, self.reward, self.done = (np.stack([r[i] for r in rows]) for i in range(4))
        self.a_next = ol.synthetic_actions(n, ps, lane0, t0 + 1 + steps, o.n_actions, nthreads=nt)

    def env(self, env, kw, **more):
        e = make_env(env, kw, batch_size=self.n, seed=self.seed, lane_offset=self.lane0, reuse_buffers=True, **more)
        e.call_counter = self.t0
        assert np.array_equal(np_(e.reset()), self.ob0)
        assert np.array_equal(np_(e.state).view(np.uint32), self.st0)
        return e

    def check_cols(self, e, cols, ctx, action=True):
        if action:
            assert np.array_equal(np_(cols["action"][:self.steps]).astype(np.int32), self.action & (0xFF if self.tape is not None else -1)), ctx
        assert np.array_equal(np_(cols["ob"]).astype(np.int32), self.ob), ctx
        assert np.array_equal(np_(cols["reward"]).astype(self.reward.dtype), self.reward), ctx
        assert np.array_equal(np_(cols["done"]), self.done.astype(bool)), ctx
        assert np.array_equal(np_(e.state).view(np.uint32), self.st), ctx
        assert e.invalid_action_count() == self.bad and e.call_counter == self.t0 + 1 + self.steps, ctx

    def returns(self, discount, pitch):
        """or_batch_collect_returns over the same steps from the same reset: (acc, cnt)"""
        st = self.st0.copy()
        acc, cnt = self.ol.new_return_stats(self.n, pitch)
        self.o.batch_collect_returns(st, acc, cnt, discount, self.seed, self.lane0, self.t0 + 1, self.steps, nthreads=self.nt,
                                     actions=None if self.tape is None else self.tape.astype(np.int32))
        assert np.array_equal(st, self.st)
        return acc, cnt


# ---- collect_synthetic, columns: every kernel the launcher picks ---------------------------------------------------------------
# (env, kwargs, n, steps, coordinate sets, kernel)
COLUMNS = [
    ("rock", {}, 3 << 18, 20, KS, "steps_quad_kernel<RockEnv<1>>"),
    ("rock", {}, 1 << 19, 20, ("K1",), "steps_kernel<RockEnv<1>, 2, true>"),
    ("rock", {}, (1 << 19) + 4, 20, ("K1",), "steps_kernel<RockEnv<1>, 2, false>"),
    ("rock", {}, 1 << 17, 20, ("K1",), "steps_kernel<RockEnv<1>, 1, true, true>"),          # the table-driven step
    ("rock", {}, 1 << 17, 8, ("K1",), "steps_kernel<RockEnv<1>, 1, true>"),                 # short: the arithmetic step
    ("rock", {}, 1 << 20, 5, ("K1",), "steps_kernel<RockEnv<1>, 4, true>"),
    ("rock", ROCK15, 3 << 18, 20, KS, "steps_quad_kernel<RockEnv<2>>"),
    ("stochrock", {}, 1 << 19, 20, KS, "steps_quad_kernel<StochasticRockEnv<1>>"),          # gate_fx as well as sensor_fx
    ("stochrock", {}, 1 << 18, 20, ("K1",), "steps_kernel<StochasticRockEnv<1>, 1, true>"),
    ("tag", {}, 1 << 19, 20, KS, "tag_steps_quad_kernel<true>"),
    ("tag", {}, 1 << 19, 8, ("K1",), "tag_steps_quad_kernel<false>"),
    ("tag", {}, 1 << 18, 20, ("K1",), "steps_kernel<TagEnv, 1, true>"),
    ("tag", dict(num_opponents=2), 1 << 19, 20, ("K1",), "steps_kernel<TagEnv, 2, true>"),
    ("tiger", {}, 1 << 19, 20, KS, "steps_quad_generic_kernel<TigerEnv>"),
    ("tiger", {}, 1 << 18, 20, ("K1",), "steps_kernel<TigerEnv, 1, true>"),
    ("network", {}, 1 << 19, 20, KS, "network_steps_quad_kernel<2, Columns, true>"),
    ("network", NET16, 1 << 19, 20, KS, "network_steps_quad_kernel<2, Columns, false>"),
    ("network", {}, 1 << 18, 20, ("K1",), "steps_kernel<NetworkEnv, 1, true>"),
    # three launches of at most 64 steps: boards dealt in one launch are used up in the next, stream NEXT at a carried counter
    ("battleship", {}, 1 << 16, 130, KS, "battleship_steps_quad_kernel<BattleShipEnv<1>>"),
    ("battleship", {}, 1 << 15, 130, ("K1",), "steps_kernel<BattleShipEnv<1>, 1, true>"),
    # ragged batches.  lane0 has to be a multiple of 4: with n % 4 == 3 the batch's last quad is the top one, its last lane
    # 0xFFFFFFFE and the padding thread's 0xFFFFFFFF; with n % 4 == 0 and a ragged last workgroup the last lane is 0xFFFFFFFF and
    # the idle threads' lane ids wrap
    ("rock", {}, 4099, 20, ("K1",), "steps_kernel<RockEnv<1>, 1, false>"),
    ("rock", {}, 4100, 20, ("K1",), "steps_kernel<RockEnv<1>, 1, false>"),
    ("tiger", {}, 3, 20, ("K1",), "steps_kernel<TigerEnv, 1, false>"),
]
COLUMN_CASES = [c[:4] + (K, c[5]) for c in COLUMNS for K in c[4]]


@pytest.mark.parametrize("env,kw,n,steps,K,kernel", COLUMN_CASES, ids=["%s%s-%d-%d-%s" % (c[0], kwid(c[1]), c[2], c[3], c[4]) for c in COLUMN_CASES])
def test_collected_columns_equal_the_oracle(oracle_lib, fuse64, env, kw, n, steps, K, kernel):
    """collect_synthetic(steps): every row of every column over the whole batch, the row of next actions, the final state."""
    seed, lane0, t0 = coords(K, n)
    if K == "K1":
        assert lane0 + (n + 3) // 4 * 4 == 1 << 32 and (t0 < 1 << 32 <= t0 + steps or steps < 8)
    r = Ref(oracle_lib, env, kw, n, steps, seed, lane0, t0)
    e = r.env(env, kw)
    tr = e.collect_synthetic(steps)
    ctx = (env, kw, n, steps, K)
    r.check_cols(e, tr, ctx)
    assert np.array_equal(np_(tr["action"][steps]), r.a_next), ctx
    assert last_kernel() == kernel, ctx
    if env != "network":
        assert r.done.any(), ctx                                         # episodes ended and restarted inside the launch


# ---- the other sinks, at each env's quad gate and one size below it ------------------------------------------------------------
GATES = [("rock", {}, 3 << 18), ("stochrock", {}, 1 << 19), ("tag", {}, 1 << 19), ("tiger", {}, 1 << 19), ("network", {}, 1 << 19),
         ("battleship", {}, 1 << 16)]
QUAD = {"rock": "steps_quad_kernel<RockEnv<1>", "stochrock": "steps_quad_kernel<StochasticRockEnv<1>", "tag": "tag_steps_quad_kernel<true",
        "tiger": "steps_quad_generic_kernel<TigerEnv", "battleship": "battleship_steps_quad_kernel<BattleShipEnv<1>"}
GATE_COLUMNS = {"rock": "steps_quad_kernel<RockEnv<1>>", "stochrock": "steps_quad_kernel<StochasticRockEnv<1>>",
                "tag": "tag_steps_quad_kernel<true>", "tiger": "steps_quad_generic_kernel<TigerEnv>",
                "network": "network_steps_quad_kernel<2, Columns, true>", "battleship": "battleship_steps_quad_kernel<BattleShipEnv<1>>"}
SINK_CASES = [(env, kw, n, K, True) for env, kw, n in GATES for K in KS] + [(env, kw, n - 2048, "K1", False) for env, kw, n in GATES]
STEPS = 20


def want_kernel(env, n, at_gate, sink, taped, name):
    """At the gate: the env's quad-per-thread loop with that sink (Tag's 4-byte and returns sinks ride its half-quad form up to
    3 * 2^18 lanes).  Below it: a one- / two-lanes-per-thread loop, or the half-quad form of a quad loop."""
    tail = ", %s%s" % (sink, ", Tape" if taped else "")
    if not at_gate:
        return name.startswith("steps_kernel<") and name.endswith(tail + ">") or name.endswith(tail + ", 2>")
    if env == "network":
        return name == "network_steps_quad_kernel<2, %s, true%s>" % (sink, ", Tape" if taped else "")
    half = ", 2" if env == "tag" and sink != "Blocked" else ""
    return name == QUAD[env] + tail + half + ">"


@pytest.mark.parametrize("env,kw,n,K,at_gate", SINK_CASES, ids=["%s-%d-%s" % (c[0], c[2], c[3]) for c in SINK_CASES])
def test_other_sinks_equal_the_oracle(oracle_lib, env, kw, n, K, at_gate):
    """packed, blocked and narrow trajectories, the returns sink (against or_batch_collect_returns) and
    rollout_synthetic(fuse=True), 20 steps in one launch: one oracle pass, one env per sink."""
    seed, lane0, t0 = coords(K, n)
    r = Ref(oracle_lib, env, kw, n, STEPS, seed, lane0, t0)
    for layout in ("packed", "blocked", "narrow"):
        e = r.env(env, kw)
        tr = e.collect_synthetic(STEPS, layout=layout)
        name = last_kernel()
        r.check_cols(e, e.decode_trajectory(tr), (env, n, K, layout))
        assert want_kernel(env, n, at_gate, layout.capitalize(), False, name), (env, n, K, layout, name)
    e = r.env(env, kw)
    stats = e.collect_returns(STEPS)
    name = last_kernel()
    acc, cnt = r.returns(e._discount, stats.acc.shape[1])
    assert np.array_equal(np_(stats.acc)[:, :n].view(np.uint64), acc[:, :n].view(np.uint64)), (env, n, K)
    assert np.array_equal(np_(stats.cnt)[:, :n], cnt[:, :n]) and np.array_equal(np_(e.state).view(np.uint32), r.st), (env, n, K)
    assert want_kernel(env, n, at_gate, "Returns", False, name), (env, n, K, name)
    e = r.env(env, kw)
    ob, rew, done = e.rollout_synthetic(STEPS, fuse=True)
    ctx = (env, n, K, "fused overwrite")
    assert np.array_equal(np_(ob), r.ob[-1]) and np.array_equal(np_(rew), r.reward[-1]) and np.array_equal(np_(done), r.done[-1].astype(bool)), ctx
    assert np.array_equal(np_(e._action_scratch), r.a_next) and np.array_equal(np_(e.state).view(np.uint32), r.st), ctx
    assert last_kernel() == GATE_COLUMNS[env] if at_gate else last_kernel().startswith("steps_kernel<"), (ctx, last_kernel())


@pytest.mark.parametrize("env,kw,n,K,at_gate", SINK_CASES, ids=["%s-%d-%s" % (c[0], c[2], c[3]) for c in SINK_CASES])
def test_tape_driven_sinks_equal_the_oracle(oracle_lib, env, kw, n, K, at_gate):
    """collect_tape in packed and returns form: the env's draws at these coordinates on the caller's actions (one lane-step in
    4096 out of range)."""
    seed, lane0, t0 = coords(K, n)
    o = oracle_lib.OracleEnv(env, **kw)
    tape = _tape(np.random.RandomState(n % 9973 + len(K)), o.n_actions, STEPS, n, 4096)
    d_tape = torch.as_tensor(tape, device="cuda")
    r = Ref(oracle_lib, env, kw, n, STEPS, seed, lane0, t0, tape=tape)
    e = r.env(env, kw)
    tr = e.collect_tape(d_tape, layout="packed")
    name = last_kernel()
    r.check_cols(e, e.decode_trajectory(tr, STEPS), (env, n, K, "tape packed"))
    assert r.bad == int((tape >= o.n_actions).sum()) > 0
    assert want_kernel(env, n, at_gate, "Packed", True, name), (env, n, K, name)
    e = r.env(env, kw)
    stats = e.collect_tape(d_tape, layout="returns")
    name = last_kernel()
    acc, cnt = r.returns(e._discount, stats.acc.shape[1])
    assert np.array_equal(np_(stats.acc)[:, :n].view(np.uint64), acc[:, :n].view(np.uint64)), (env, n, K)
    assert np.array_equal(np_(stats.cnt)[:, :n], cnt[:, :n]) and np.array_equal(np_(e.state).view(np.uint32), r.st), (env, n, K)
    assert e.invalid_action_count() == r.bad
    assert want_kernel(env, n, at_gate, "Returns", True, name), (env, n, K, name)


@pytest.mark.parametrize("env,kw,n", [("rock", {}, 1 << 19), ("tag", {}, 1 << 18), ("network", {}, 1 << 19), ("battleship", {}, 1 << 16),
                                      ("tiger", {}, 4100)], ids=["rock", "tag", "network", "battleship", "tiger-ragged"])
def test_a_policy_key_that_differs_in_its_high_word_only(oracle_lib, env, kw, n):
    """rollout_synthetic(action_seed = seed ^ 2^32): policy and env no longer share a key, so the plain launches run (a policy
    launch and a step launch per step) and the results are the oracle's fed synthetic_actions(seed ^ 2^32).  A launcher that
    compared the low key words only would chain them."""
    seed, lane0, t0 = coords("K1", n)
    other = seed ^ 1 << 32
    steps = 9
    r = Ref(oracle_lib, env, kw, n, steps, seed, lane0, t0, pol_seed=other)
    same = oracle_lib.synthetic_actions(n, seed, lane0, t0 + 1, r.o.n_actions)
    assert not np.array_equal(same, r.action[0])
    for fuse in (False, True):                                           # (fusing needs the shared key: the flag changes nothing here)
        e = r.env(env, kw)
        ob, rew, done = e.rollout_synthetic(steps, action_seed=other, fuse=fuse)
        assert np.array_equal(np_(ob), r.ob[-1]) and np.array_equal(np_(rew), r.reward[-1]) and np.array_equal(np_(done), r.done[-1].astype(bool))
        assert np.array_equal(np_(e._action_scratch), r.a_next) and np.array_equal(np_(e.state).view(np.uint32), r.st)
        assert e.invalid_action_count() == 0 and e.call_counter == t0 + 1 + steps


# ---- single steps ----------------------------------------------------------------------------------------------------------------
STEP_CASES = [("rock", {}, 1 << 19, K) for K in KS] + [("network", {}, 1 << 19, K) for K in KS] + \
             [("rock", ROCK15, 1 << 19, "K1"), ("stochrock", {}, 1 << 19, "K1"), ("tag", {}, 1 << 19, "K1"), ("tiger", {}, 1 << 19, "K1"),
              ("battleship", {}, 1 << 18, "K1"), ("rock", {}, 1 << 18, "K1"), ("rock", {}, 4099, "K1"), ("network", {}, 4100, "K1")]


@pytest.mark.parametrize("env,kw,n,K", STEP_CASES, ids=["%s%s-%d-%s" % (c[0], kwid(c[1]), c[2], c[3]) for c in STEP_CASES])
def test_single_steps_and_resets_equal_the_oracle(oracle_lib, env, kw, n, K):
    """reset(), nine step() calls (2^19 lanes: step_quad_kernel / network_step_quad_kernel; 2^18: two lanes per thread; ragged:
    one), a masked reset and another step, row by row — the call counter carries between two launches here."""
    seed, lane0, t0 = coords(K, n)
    nt = oracle_lib.max_threads()
    o = oracle_lib.OracleEnv(env, **kw)
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
    e.call_counter = t0
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, t0, nthreads=nt))
    done = np.zeros(n, np.uint8)

    def step():
        t = e.call_counter
        a = oracle_lib.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt)
        assert np.array_equal(np_(e.synthetic_actions()), a), (env, n, K, t)
        ob, rew, d, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
        g_ob, g_rew, g_done, _ = e.step(torch.as_tensor(a, device="cuda"))
        assert bad == 0 and np.array_equal(np_(g_ob), ob) and np.array_equal(np_(g_rew), rew), (env, n, K, t)
        assert np.array_equal(np_(g_done), d.astype(bool)) and np.array_equal(np_(e.state).view(np.uint32), st), (env, n, K, t)

    for _ in range(9):
        step()
    mask = np.random.RandomState(3).rand(n) < .4
    t = e.call_counter
    fresh = o.new_state(n)
    want_ob = o.batch_reset(fresh, seed, lane0, t, nthreads=nt)
    ob = e.reset(where=torch.as_tensor(mask, device="cuda"))
    st[:] = np.where(mask[None, :], fresh, st)
    assert np.array_equal(np_(ob), np.where(mask, want_ob, -1)) and np.array_equal(np_(e.state).view(np.uint32), st)
    done[:] = 0
    step()


# ---- episodes played to their end ------------------------------------------------------------------------------------------------
EPISODE_CASES = [("rock", {}, 4099, "K1", "episodes_kernel<"), ("tag", {}, 4100, "K1", "episodes_kernel<"),
                 ("battleship", {}, 4099, "K1", "episodes_kernel<"), ("tiger", {}, 4099, "K1", "episodes_kernel<"),
                 ("network", {}, 4100, "K1", "episodes_kernel<")] + \
                [("rock", {}, 3 << 18, K, "episodes_quad_kernel<RockEnv<1>, ") for K in KS] + \
                [("stochrock", {}, 1 << 19, K, "episodes_quad_kernel<StochasticRockEnv<1>, ") for K in KS] + \
                [("rock", ROCK15, 3 << 18, "K1", "episodes_quad_kernel<RockEnv<2>, ")]


@pytest.mark.parametrize("policy", ["synthetic", "tape"])
@pytest.mark.parametrize("env,kw,n,K,kernel", EPISODE_CASES, ids=["%s%s-%d-%s" % (c[0], kwid(c[1]), c[2], c[3]) for c in EPISODE_CASES])
def test_finish_reset_finish_equals_the_oracle(oracle_lib, env, kw, n, K, kernel, policy):
    """finish_episodes from a state with frozen lanes (every sink, both kernels of episodes.hip), reset(where=done), then
    finish_episodes again: rows, statistics, state and done flags."""
    seed, lane0, t0 = coords(K, n)
    k = 20
    p = Pair(oracle_lib, env, kw, n, lane0, pre_steps=2, seed=seed, t0=t0)
    tape = random_tape(p.o, k, n, 11) if policy == "tape" else None
    act = None if tape is None else torch.as_tensor(tape, device="cuda")
    snap = p.snapshot()
    rows, bad = p.oracle_rows(k, tape)
    want_st, want_done = p.st.copy(), p.done.copy()
    codes = None
    for layout in ("packed", "narrow", "returns"):
        p.restore(snap)
        p.e._err.zero_()
        out = p.e.finish_episodes(k, actions=act, layout=layout)
        ctx = (env, kw, n, K, policy, layout)
        assert last_kernel().startswith(kernel) if kernel.startswith("episodes_quad") else kernel in last_kernel(), (ctx, last_kernel())
        if layout != "returns":
            check_rows(p, out, rows, ctx)
            if layout == "packed":
                codes = (np_(out["traj"]) >> 16) & 0xFF
        else:
            check_returns(p, out, [(a, ob, rw, d, codes[s][:n]) for s, (a, ob, rw, d) in enumerate(rows)], snap[4], ctx)
        assert np.array_equal(np_(p.e.state).view(np.uint32), want_st) and np.array_equal(np_(p.e._done), want_done), ctx
        assert p.e.invalid_action_count() == bad and p.e.call_counter == snap[2] + k, ctx
    p.st, p.done = want_st, want_done
    mask = p.done.astype(bool)
    assert mask.any()
    t = p.e.call_counter
    ob = p.e.reset(where=p.e.done)
    fresh = p.o.new_state(n)
    want_ob = p.o.batch_reset(fresh, seed, lane0, t, nthreads=p.nt)
    p.st = np.where(mask[None, :], fresh, p.st).astype(np.uint32)
    p.done = np.zeros(n, np.uint8)
    assert np.array_equal(np_(ob), np.where(mask, want_ob, -1))
    p.check_state()
    snap = p.snapshot()
    rows, bad = p.oracle_rows(k, tape)
    want_st = p.st.copy()
    p.restore(snap)
    p.e._err.zero_()
    out = p.e.finish_episodes(k, actions=act, layout="narrow")
    check_rows(p, out, rows, (env, kw, n, K, policy, "again"))
    assert np.array_equal(np_(p.e.state).view(np.uint32), want_st) and p.e.invalid_action_count() == bad


# ---- the heuristic-policy loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 1031], ids=["full", "ragged"])
@pytest.mark.parametrize("env,kw,max_size", [("rock", dict(board_size=7, num_rocks=8), None), ("rock", dict(board_size=7, num_rocks=8), 6),
                                             ("tag", {}, None)], ids=["rock", "rock-ring6", "tag"])
def test_heuristic_steps_equal_the_oracle(oracle_lib, env, kw, max_size, n):
    """heuristic_steps(h, 20) then (h, 5): the policy's quad-shared block, RockSample's sensor blocks and the quad transposes of a
    ragged last quad at the top of the lane range, across the carry of the call counter."""
    seed, lane0, t0 = coords("K1", n)
    _heuristic_fused_vs_oracle(oracle_lib, env, kw, n, (20, 5), seed=seed, lane0=lane0, max_size=max_size, t0=t0)


# ---- the planner -----------------------------------------------------------------------------------------------------------------
ROOTS, SIMS, DEPTH = 64, 64, 16
PLAN_CASES = [(env, kw, K) for env, kw in (("rock", {}), ("tag", {}), ("battleship", {})) for K in KS]


@pytest.mark.parametrize("env,kw,K", PLAN_CASES, ids=["%s-%s" % (c[0], c[2]) for c in PLAN_CASES])
def test_rollout_plan_and_plan_step_equal_the_oracle(oracle_lib, env, kw, K):
    """rollout_kernel (t0 + step inside the launch): 64 roots x 64 simulations x 16 steps whose last simulation is global lane
    0xFFFFFFFF under K1 ((lane_offset + roots) * sims == 2^32) — every simulation's return (float64), length, first action, last
    observation and termination; then plan()'s action values and plan_step()'s real step."""
    ol = oracle_lib
    seed, sim_lane0, t0 = coords(K, ROOTS * SIMS)
    root_lane0 = sim_lane0 // SIMS
    if K == "K1":
        assert (root_lane0 + ROOTS) * SIMS == 1 << 32
    nt = ol.max_threads()
    o = ol.OracleEnv(env, **kw)
    e = make_env(env, kw, batch_size=ROOTS, seed=seed, lane_offset=root_lane0)
    e.call_counter = t0
    st = o.new_state(ROOTS)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, root_lane0, t0, nthreads=nt))
    t = e.call_counter
    want = o.batch_rollout(st, SIMS, DEPTH, e._discount, seed, sim_lane0, t, nthreads=nt)
    got = e.rollout(DEPTH, sims_per_root=SIMS, lane_offset=sim_lane0)
    assert np.array_equal(np_(got["ret"]).view(np.uint64), want["ret"].view(np.uint64)), (env, K)
    for k in ("n_steps", "first_action", "last_ob"):
        assert np.array_equal(np_(got[k]), want[k]), (env, K, k)
    assert np.array_equal(np_(got["terminated"]), want["terminated"].astype(bool))
    assert int(want["n_steps"].sum()) > ROOTS * SIMS and len(np.unique(want["first_action"])) > 1
    for real_step in (False, True):
        t = e.call_counter
        r = o.batch_rollout(st, SIMS, DEPTH, e._discount, seed, sim_lane0, t, nthreads=nt)
        w = ol.plan_reduce(r["ret"], r["first_action"], ROOTS, SIMS, o.n_actions)
        if real_step:
            ob, rew, done, _, plan = e.plan_step(DEPTH, sims_per_root=SIMS)
        else:
            plan = e.plan(DEPTH, sims_per_root=SIMS)
        assert np.array_equal(np_(plan["sim_ret"]).view(np.uint64), r["ret"].view(np.uint64)), (env, K, real_step)
        assert np.array_equal(np_(plan["q"]).view(np.uint64), w["q"].view(np.uint64)), (env, K, real_step)
        assert np.array_equal(np_(plan["visits"]), w["visits"]) and np.array_equal(np_(plan["best"]), w["best"]), (env, K, real_step)
        if real_step:
            ob_o, rew_o, done_o, _ = o.batch_step(st, w["best"], seed, root_lane0, t + DEPTH, auto_reset=True, nthreads=nt)
            assert np.array_equal(np_(ob), ob_o) and np.array_equal(np_(rew), rew_o) and np.array_equal(np_(done), done_o.astype(bool))
            assert np.array_equal(np_(e.state).view(np.uint32), st)
