"""Episodes played to their end (ABI 15): the masked reset (reset(where=...), pomdp_reset_where) and the frozen-lane fused loops
(finish_episodes, pomdp_finish_episodes) against the CPU oracle stepped with auto_reset=False, row by row."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV_IDS = {"rock": "Rock-v0", "stochrock": "StochasticRock-v0", "tag": "Tag-v0", "battleship": "Battleship-v0", "tiger": "Tiger-v0",
           "network": "Network-v0"}
CASES = [("rock", {}), ("rock", dict(board_size=15, num_rocks=15)), ("stochrock", {}), ("tag", {}), ("tag", dict(num_opponents=4)),
         ("battleship", {}), ("battleship", dict(board_size=(10, 10), max_len=5)), ("tiger", {}), ("network", {}),
         ("network", dict(n_machines=31))]
IDS = ["%s%s" % (c[0], "-".join(str(v) for v in c[1].values())) for c in CASES]
SEED = 77031


def make_env(env, kw, **batch):
    import gym_pomdp_amd as gpa
    return gpa.make(ENV_IDS[env], **kw, **batch)


def np_(t):
    return t.detach().cpu().numpy()


def f64_reward(env, code):
    """the reference's float64 reward of a packed record's reward code (what the returns sink adds up)"""
    code = int(code) & 0xFF
    if env != "network":
        return float(np.int8(np.uint8(code)))
    kind, base = divmod(code, 68)
    return float(base) - (0.0, .1, 2.5)[kind]


class Pair(object):
    """the GPU env (auto_reset=False) and the oracle on the same lanes, stepped into a state where some lanes are done"""

    def __init__(self, ol, env, kw, n, lane0, pre_steps=6, seed=SEED, force_done=0.25, t0=0):
        self.ol, self.env, self.kw, self.n, self.lane0, self.seed = ol, env, kw, n, lane0, seed
        self.nt = ol.max_threads()
        self.o = ol.OracleEnv(env, **kw)
        self.e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, auto_reset=False)
        self.e.call_counter = t0                                       # reset() is call t0
        self.st = self.o.new_state(n)
        ob = self.o.batch_reset(self.st, seed, lane0, t0, nthreads=self.nt)
        assert np.array_equal(np_(self.e.reset()), ob)
        self.done = np.zeros(n, np.uint8)
        for _ in range(pre_steps):
            self.step_both()
        rng = np.random.RandomState((n + lane0) & 0xFFFFFFFF)
        forced = (rng.rand(n) < force_done).astype(np.uint8)           # frozen lanes whatever their state: `done` is an input flag
        self.done |= forced
        self.e._done.copy_(torch.as_tensor(self.done, device=self.e.device))
        self.check_state()

    def actions(self, t):
        return self.ol.synthetic_actions(self.n, self.seed, self.lane0, t, self.o.n_actions)

    def step_both(self):
        t = self.e.call_counter
        a = self.actions(t)
        self.o.batch_step(self.st, a, self.seed, self.lane0, t, auto_reset=False, done=self.done, nthreads=self.nt)
        self.e.step(torch.as_tensor(a, device=self.e.device))

    def check_state(self):
        assert np.array_equal(np_(self.e.state).view(np.uint32), self.st), (self.env, self.kw)
        assert np.array_equal(np_(self.e._done), self.done), (self.env, self.kw)

    def snapshot(self):
        return self.e._state.clone(), self.e._done.clone(), self.e.call_counter, self.st.copy(), self.done.copy()

    def restore(self, snap):
        self.e._state.copy_(snap[0]); self.e._done.copy_(snap[1]); self.e.call_counter = snap[2]
        self.st, self.done = snap[3].copy(), snap[4].copy()

    def oracle_rows(self, k, tape=None):
        """k frozen-mode steps of the oracle: [(action, ob, reward, done)] per step, and the out-of-range bytes it counted"""
        rows, bad = [], 0
        t0 = self.e.call_counter
        for s in range(k):
            a = self.actions(t0 + s) if tape is None else tape[s].astype(np.int32)
            ob, rw, d, b = self.o.batch_step(self.st, a, self.seed, self.lane0, t0 + s, auto_reset=False, done=self.done, nthreads=self.nt)
            rows.append((a.copy(), ob.copy(), rw.copy(), d.copy()))
            bad += b
        return rows, bad


def random_tape(o, k, n, seed):
    rng = np.random.RandomState(seed)
    tape = rng.randint(0, o.n_actions, (k, n)).astype(np.uint8)
    bad = rng.randint(0, 23, (k, n)) == 0
    tape[bad] = rng.randint(o.n_actions, 256, int(bad.sum())).astype(np.uint8)
    return tape


def reduce_returns(env, rows, done0, discount, n):
    """the returns sink's statistics from fresh ones, by a float64 restatement over the oracle's rows in the stated order
    (rows: (action, ob, reward, done, reward code) per step; done0: the done flags the call started from)"""
    ret, disc = np.zeros(n), np.ones(n)
    ret_done, ret_sum = np.full(n, np.nan), np.zeros(n)
    eps, steps = np.zeros(n, np.int64), np.zeros(n, np.int64)
    was_done = done0
    for s, (a, ob, rw, d, codes) in enumerate(rows):
        live = ~was_done.astype(bool)
        for i in np.nonzero(live)[0]:
            ret[i] = ret[i] + disc[i] * f64_reward(env, codes[i])
            disc[i] = disc[i] * discount
            steps[i] += 1
            if d[i] and env != "network":
                ret_done[i] = ret[i]; ret_sum[i] = ret_sum[i] + ret[i]; eps[i] += 1
                ret[i], disc[i] = 0.0, 1.0
        was_done = d
    return ret, disc, ret_done, ret_sum, eps, steps


def check_rows(p, out, rows, ctx):
    dec = p.e.decode_trajectory(out)
    for s, (a, ob, rw, d) in enumerate(rows):
        assert np.array_equal(np_(dec["action"][s]).astype(np.int64), a.astype(np.int64) & 0xFF), ctx + (s, "action")
        assert np.array_equal(np_(dec["ob"][s]).astype(np.int64), ob), ctx + (s, "ob")
        assert np.array_equal(np_(dec["reward"][s]).astype(np.float64), rw.astype(np.float64)), ctx + (s, "reward")
        assert np.array_equal(np_(dec["done"][s]).astype(np.uint8), d), ctx + (s, "done")


# ---- 1. masked reset ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lane0", [(4099, 4096), (1 << 16, 0)])
@pytest.mark.parametrize("env,kw", CASES, ids=IDS)
def test_masked_reset_equals_the_oracle(oracle_lib, env, kw, n, lane0):
    p = Pair(oracle_lib, env, kw, n, lane0)
    rng = np.random.RandomState(5)
    mask = rng.rand(n) < .4
    t = p.e.call_counter
    fresh = p.o.new_state(n)
    want_ob = p.o.batch_reset(fresh, p.seed, lane0, t, nthreads=p.nt)
    prev = np_(p.e.state).view(np.uint32).copy()
    prev_done = p.done.copy()
    ob = p.e.reset(where=torch.as_tensor(mask, device="cuda"))
    assert p.e.call_counter == t + 1
    assert np.array_equal(np_(ob), np.where(mask, want_ob, -1))
    assert np.array_equal(np_(p.e.state).view(np.uint32), np.where(mask[None, :], fresh, prev))
    assert np.array_equal(np_(p.e._done), np.where(mask, 0, prev_done))
    assert torch.equal(p.e.done, p.e._done.view(torch.bool))
    # an empty mask changes nothing but the counter; an all-ones mask is reset()
    st1, d1 = p.e.state.clone(), p.e._done.clone()
    assert (np_(p.e.reset(where=np.zeros(n, bool))) == -1).all() and p.e.call_counter == t + 2
    assert torch.equal(p.e.state, st1) and torch.equal(p.e._done, d1)
    t = p.e.call_counter
    ob_all = p.e.reset(where=np.ones(n, np.uint8))
    q = make_env(env, kw, batch_size=n, seed=p.seed, lane_offset=lane0, auto_reset=False)
    q.call_counter = t
    assert torch.equal(ob_all, q.reset()) and torch.equal(p.e.state, q.state) and not bool(p.e._done.any())


def test_masked_reset_of_a_scalar_env():
    e = make_env("tiger", {}, seed=3)
    ob = e.reset()
    t = e.call_counter
    assert e.reset(where=[False]) == -1 and e.call_counter == t + 1
    q = make_env("tiger", {}, seed=3)
    q.call_counter = t + 1
    assert e.reset(where=[True]) == q.reset() and e.done is False and isinstance(ob, int)


# ---- 2. frozen rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["synthetic", "tape"])
@pytest.mark.parametrize("env,kw", CASES, ids=IDS)
def test_frozen_rows_equal_the_oracle(oracle_lib, env, kw, policy):
    from gym_pomdp_amd import _native
    n, lane0, k = 4099, 4096, 37
    p = Pair(oracle_lib, env, kw, n, lane0)
    tape = random_tape(p.o, k, n, 11) if policy == "tape" else None
    snap = p.snapshot()
    rows, bad = p.oracle_rows(k, tape)
    want_st, want_done = p.st.copy(), p.done.copy()
    for layout in ("packed", "narrow"):
        p.restore(snap)
        p.e._err.zero_()
        out = p.e.finish_episodes(k, actions=None if tape is None else torch.as_tensor(tape, device="cuda"), layout=layout)
        ctx = (env, kw, policy, layout)
        assert "episodes_kernel<" in _native.lib().pomdp_last_fused_kernel().decode(), ctx
        check_rows(p, out, rows, ctx)
        assert np.array_equal(np_(p.e.state).view(np.uint32), want_st), ctx
        assert np.array_equal(np_(p.e._done), want_done) and torch.equal(p.e.done, p.e._done.view(torch.bool)), ctx
        assert p.e.invalid_action_count() == bad and (policy == "synthetic") == (bad == 0), ctx
        assert p.e.call_counter == snap[2] + k, ctx


@pytest.mark.slow
@pytest.mark.parametrize("policy", ["synthetic", "tape"])
@pytest.mark.parametrize("env,kw", [("rock", {}), ("rock", dict(board_size=15, num_rocks=15)), ("stochrock", {})], ids=["rock", "rock15", "stochrock"])
def test_frozen_rows_of_the_quad_loop(oracle_lib, env, kw, policy):
    """2^20 lanes: RockSample's quad-per-thread frozen loop, every sink, against the oracle"""
    from gym_pomdp_amd import _native
    n, lane0, k = 1 << 20, 0, 40
    p = Pair(oracle_lib, env, kw, n, lane0, pre_steps=8)
    tape = random_tape(p.o, k, n, 12) if policy == "tape" else None
    snap = p.snapshot()
    rows, bad = p.oracle_rows(k, tape)
    want_st, want_done = p.st.copy(), p.done.copy()
    name = "episodes_quad_kernel<%s<%d>, " % ("StochasticRockEnv" if env == "stochrock" else "RockEnv", 2 if kw else 1)
    for layout in ("packed", "narrow", "returns"):
        p.restore(snap)
        p.e._err.zero_()
        out = p.e.finish_episodes(k, actions=None if tape is None else torch.as_tensor(tape, device="cuda"), layout=layout)
        ctx = (env, kw, policy, layout)
        assert _native.lib().pomdp_last_fused_kernel().decode().startswith(name), (ctx, _native.lib().pomdp_last_fused_kernel())
        if layout != "returns":
            check_rows(p, out, rows, ctx)
            codes = (np_(out["traj"] if layout == "packed" else out["traj"][:, 2].to(torch.int32)) >> (16 if layout == "packed" else 0)) & 0xFF
        else:
            full = [(a, ob, rw, d, codes[s][:n]) for s, (a, ob, rw, d) in enumerate(rows)]
            check_returns(p, out, full, snap[4], ctx)
        assert np.array_equal(np_(p.e.state).view(np.uint32), want_st), ctx
        assert np.array_equal(np_(p.e._done), want_done), ctx
        assert p.e.invalid_action_count() == bad, ctx


def check_returns(p, stats, full, done0, ctx):
    ret, disc, ret_done, ret_sum, eps, steps = reduce_returns(p.env, full, done0, p.e._discount, p.n)
    for got, want, name in ((stats.ret, ret, "ret"), (stats.disc, disc, "disc"), (stats.ret_done, ret_done, "ret_done"),
                            (stats.ret_sum, ret_sum, "ret_sum")):
        if p.env == "network" and name in ("ret_done", "ret_sum"):
            continue
        assert np.array_equal(np_(got).view(np.uint64), want.view(np.uint64)), ctx + (name,)
    assert np.array_equal(np_(stats.steps), steps), ctx
    if p.env != "network":
        assert np.array_equal(np_(stats.episodes), eps), ctx


# ---- 3. returns sink ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["synthetic", "tape"])
@pytest.mark.parametrize("env,kw", CASES, ids=IDS)
def test_returns_sink_equals_a_float64_reduction_of_the_rows(oracle_lib, env, kw, policy):
    n, lane0, k = 4099, 4096, 41
    p = Pair(oracle_lib, env, kw, n, lane0)
    tape = random_tape(p.o, k, n, 13) if policy == "tape" else None
    act = None if tape is None else torch.as_tensor(tape, device="cuda")
    snap = p.snapshot()
    rows, _ = p.oracle_rows(k, tape)
    want_st = p.st.copy()
    p.restore(snap)
    traj = p.e.finish_episodes(k, actions=act, layout="packed")
    codes = (np_(traj["traj"]) >> 16) & 0xFF
    p.restore(snap)
    stats = p.e.finish_episodes(k, actions=act)
    full = [(a, ob, rw, d, codes[s][:n]) for s, (a, ob, rw, d) in enumerate(rows)]
    check_returns(p, stats, full, snap[4], (env, kw, policy))
    assert np.array_equal(np_(p.e.state).view(np.uint32), want_st)


@pytest.mark.parametrize("env,kw,k", [("rock", {}, 64), ("tag", {}, 64), ("tiger", {}, 3), ("battleship", {}, 64)],
                         ids=["rock", "tag", "tiger", "battleship"])
def test_one_finished_episode_matches_the_auto_reset_returns(env, kw, k):
    """where the auto-reset collect_returns over the same k steps from a fresh reset() finishes exactly one episode for a lane,
    that episode's return equals the frozen loop's ret_done (Tiger's episodes end within a few steps: k = 3)"""
    n, seed = 1 << 14, 99
    a = make_env(env, kw, batch_size=n, seed=seed, auto_reset=True)
    a.reset()
    sa = a.collect_returns(k)
    f = make_env(env, kw, batch_size=n, seed=seed, auto_reset=False)
    f.reset()
    sf = f.finish_episodes(k)
    one = sa.episodes == 1
    assert int(one.sum()) > 0
    assert torch.equal(sa.ret_done[one], sf.ret_done[one])
    assert bool((sf.episodes <= 1).all()) and torch.equal(sf.episodes.bool(), f.done)


# ---- 4. invariance -----------------------------------------------------------------------------------------------------------
CUTS = [("rock", {}, 4099), ("stochrock", {}, 4099), ("tag", {}, 4099), ("network", {}, 4099), ("battleship", {}, 4099),
        ("rock", {}, 1 << 20), ("stochrock", {}, 1 << 20)]       # 2^20: RockSample's quad loop, its two shards the general one


@pytest.mark.parametrize("env,kw,n", CUTS, ids=["%s-%d" % (c[0], c[2]) for c in CUTS])
def test_results_do_not_depend_on_how_the_steps_are_cut(env, kw, n):
    from gym_pomdp_amd import _native
    L = _native.lib()
    k1, k2, seed = 20, 29, 5
    outs = []
    old = L.pomdp_fuse_max(0)
    try:
        for cut in ("one", "two", "fuse7", "fuse64", "shards"):
            L.pomdp_fuse_max({"fuse7": 7, "fuse64": 64}.get(cut, old))
            parts = [(0, n)] if cut != "shards" else [(0, n // 2 // 4 * 4), (n // 2 // 4 * 4, n)]
            res = []
            for lo, hi in parts:
                e = make_env(env, kw, batch_size=hi - lo, seed=seed, lane_offset=lo, auto_reset=False)
                e.reset()
                if cut == "two":
                    st = e.finish_episodes(k1)
                    e.finish_episodes(k2, stats=st)
                else:
                    st = e.finish_episodes(k1 + k2)
                res.append((np_(e.state), np_(e._done), np_(st.acc[:, :hi - lo]), np_(st.cnt[:, :hi - lo])))
            outs.append([np.concatenate([r[i] for r in res], axis=-1) for i in range(4)])
    finally:
        L.pomdp_fuse_max(old)
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---- 5. the episode loop end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,kw", [("rock", {}), ("tiger", {}), ("battleship", {}), ("tag", dict(num_opponents=4))],
                         ids=["rock", "tiger", "battleship", "tag4"])
def test_finish_reset_finish_equals_the_oracle(oracle_lib, env, kw):
    n, lane0, k = 4099, 4096, 30
    p = Pair(oracle_lib, env, kw, n, lane0, pre_steps=0, force_done=0.0)
    p.oracle_rows(k)                                                   # (reads the env's call counter before the call moves it)
    p.e.finish_episodes(k, layout="packed")
    p.check_state()
    mask = p.done.astype(bool)
    assert mask.any()
    t = p.e.call_counter
    ob = p.e.reset(where=p.e.done)
    fresh = p.o.new_state(n)
    want_ob = p.o.batch_reset(fresh, p.seed, lane0, t, nthreads=p.nt)
    p.st = np.where(mask[None, :], fresh, p.st).astype(np.uint32)
    p.done = np.where(mask, 0, p.done).astype(np.uint8)
    assert np.array_equal(np_(ob), np.where(mask, want_ob, -1))
    p.check_state()
    snap = p.snapshot()
    rows, _ = p.oracle_rows(k)
    want_st = p.st.copy()
    p.restore(snap)
    out = p.e.finish_episodes(k, layout="narrow")
    check_rows(p, out, rows, (env, kw))
    assert np.array_equal(np_(p.e.state).view(np.uint32), want_st)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    from gym_pomdp_amd import _native
    e = make_env("rock", {}, batch_size=64, seed=1)                     # auto_reset by default
    e.reset()
    with pytest.raises(ValueError):
        e.finish_episodes(8)
    h = make_env("rock", dict(use_heuristic=True), batch_size=64, seed=1, auto_reset=False)
    h.reset()
    with pytest.raises(ValueError):
        h.finish_episodes(8)
    s = make_env("rock", {}, batch_size=64, seed=1, auto_reset=False, lane_offset=2)
    s.reset()
    with pytest.raises(ValueError):
        s.finish_episodes(8)
    f = make_env("rock", {}, batch_size=64, seed=1, auto_reset=False)
    f.reset()
    with pytest.raises(ValueError):
        f.finish_episodes(8, layout="columns")
    L = _native.lib()
    args = _native.EpisodeArgs(env=0, layout=_native.POMDP_LAYOUT_RETURNS, params=C.addressof(f._params), state=f._ptrs[0],
                               done=f._ptrs[3], n=64, seed=1, lane0=0)
    assert L.pomdp_finish_episodes(C.byref(args), 0, 8, None) == -1     # no statistics
    args.layout, args.traj, args.pitch = _native.LAYOUTS["blocked"], f._ptrs[0], 256
    assert L.pomdp_finish_episodes(C.byref(args), 0, 8, None) == -1     # no 13-byte layouts in frozen mode
    args.layout, args.pitch = _native.LAYOUTS["packed"], 16
    assert L.pomdp_finish_episodes(C.byref(args), 0, 8, None) == -1     # pitch < n
    args.pitch, args.lane0 = 64, 2
    assert L.pomdp_finish_episodes(C.byref(args), 0, 8, None) == -1     # lane0 % 4
    args.lane0, args.done = 0, None
    assert L.pomdp_finish_episodes(C.byref(args), 0, 8, None) == -1     # no done flags
    assert L.pomdp_finish_episodes(None, 0, 8, None) == -1
    assert L.pomdp_reset_where(0, C.addressof(f._params), None, None, None, None, 64, 1, 0, 0, None) == -1
