"""Finite-state controllers inside the fused loop (env.run_controller, pomdp_controller_episodes) against the contract's CPU
restatement (tests/controller_restatement.py: the oracle stepped with auto_reset=False under numpy gathers), row by row.
Every test runs 1000 lanes — three full workgroups, a partial one and a ragged last wave — from lane_offset 8."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controller_restatement as cr  # noqa: E402

pytestmark = pytest.mark.gpu

ENV_IDS = {"rock": "Rock-v0", "stochrock": "StochasticRock-v0", "tag": "Tag-v0", "battleship": "Battleship-v0", "tiger": "Tiger-v0",
           "network": "Network-v0"}
N, LANE0, SEED, NODES = 1000, 8, 12345, 128
# env -> steps per call (RockSample(7, 8), BattleShip 5 x 5: the defaults)
STEPS = {"rock": 8, "stochrock": 64, "tag": 32, "tiger": 8, "battleship": 32, "network": 16}


def np_(t):
    return t.detach().cpu().numpy()


def make_env(env, **kw):
    import gym_pomdp_amd as gpa
    return gpa.make(ENV_IDS[env], batch_size=N, seed=SEED, lane_offset=LANE0, auto_reset=False, **kw)


def random_tables(o, nodes=NODES, seed=7):
    """a seeded random controller and per-lane random start nodes"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, o.n_actions, nodes), rng.randint(0, nodes, (nodes, o.n_obs)), rng.randint(0, nodes, N)


def rows_of(out, k):
    """the packed records uint32 [k, N] of a packed or narrow trajectory"""
    if out["layout"] == "packed":
        return np_(out["traj"][:k, :N]).view(np.uint32)
    t = np_(out["traj"][:k, :, :N]).astype(np.uint32)
    return t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16) | (t[:, 3] << 24)


def same_f64(got, want):
    """bit for bit; the NaN a fresh ret_done holds equals itself"""
    return bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


class Run(object):
    """one env on the GPU and the oracle after the same reset() (call counter 0), and a controller of the GPU env"""

    def __init__(self, ol, env, action, nxt, start, validate=True, **kw):
        import gym_pomdp_amd as gpa
        self.ol, self.env, self.nt = ol, env, ol.max_threads()
        self.o = ol.OracleEnv(env, **kw)
        self.e = make_env(env, **kw)
        self.st0 = self.o.new_state(N)
        ob = self.o.batch_reset(self.st0, SEED, LANE0, 0, nthreads=self.nt)
        assert np.array_equal(np_(self.e.reset()), ob)
        self.gpu_st0 = self.e._state.clone()
        self.action, self.nxt = np.asarray(action), np.asarray(nxt)
        self.start = np.broadcast_to(np.asarray(start, np.int64), (N,)).copy()
        self.ctrl = gpa.Controller(self.e, action, nxt, start=start, validate=validate)

    def reference(self, k, calls=1):
        """[(packed, refused entries so far, state, done, node, acc, cnt)] after each of `calls` calls of k steps from t = 1"""
        st, done, node = self.st0.copy(), np.zeros(N, np.uint8), self.start.copy()
        acc, cnt = self.ol.new_return_stats(N)
        res, bad = [], 0
        for c in range(calls):
            packed, b = cr.run(self.o, st, done, node, self.action, self.nxt, k, SEED, LANE0, 1 + c * k, acc, cnt,
                               float(self.e._discount), nthreads=self.nt)
            bad += b
            res.append((packed, bad, st.copy(), done.copy(), node.copy(), acc.copy(), cnt.copy()))
        return res

    def rewind(self):
        """back to the state after reset(): call counter 1, nobody done, every lane on its start node, nothing counted"""
        self.e._state.copy_(self.gpu_st0)
        self.e._done.zero_()
        self.e._err.zero_()
        self.e.call_counter = 1
        self.ctrl.node.copy_(torch.as_tensor(self.start.astype(np.int32), device=self.e.device))

    def check(self, k, ref, layouts=("packed", "narrow", "returns")):
        """run_controller, once per entry of `ref` in a row (out / stats continued), in every layout, against `ref`"""
        from gym_pomdp_amd import _native
        for layout in layouts:
            self.rewind()
            res = None
            for c, (packed, bad, st, done, node, acc, cnt) in enumerate(ref):
                ctx = (self.env, layout, c)
                if layout == "returns":
                    res = self.e.run_controller(self.ctrl, k, stats=res)
                    assert same_f64(np_(res.acc[:, :N]), acc), ctx
                    assert np.array_equal(np_(res.cnt[:, :N]), cnt), ctx
                else:
                    res = self.e.run_controller(self.ctrl, k, layout=layout, out=res)
                    got = rows_of(res, k)
                    assert np.array_equal(got, packed), ctx + (np.argwhere(got != packed)[:4].tolist(),)
                assert _native.lib().pomdp_last_fused_kernel().decode().startswith("controller_kernel<"), ctx
                assert np.array_equal(np_(self.e.state).view(np.uint32), st), ctx
                assert np.array_equal(np_(self.e._done), done) and torch.equal(self.e.done, self.e._done.view(torch.bool)), ctx
                assert np.array_equal(np_(self.ctrl.node), node), ctx
                assert self.e.invalid_action_count() == bad, ctx
                assert self.e.call_counter == 1 + (c + 1) * k, ctx


# ---- 1. oracle parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", list(STEPS))
def test_two_calls_in_a_row_equal_the_restatement(oracle_lib, env):
    """packed rows, narrow rows, returns statistics (bit for bit), final state, done, node and the count, after each of two calls
    in a row: the second starts with frozen lanes and carried nodes.
    The share of lanes the first call finishes (from the restatement, exactly this setup): rock 0.69, stochrock 0.06, tag 0.09,
    tiger 0.96, battleship 0.03 — neither an all-live nor an all-frozen batch; Network's episodes never end."""
    k = STEPS[env]
    r = Run(oracle_lib, env, *random_tables(oracle_lib.OracleEnv(env)))
    ref = r.reference(k, calls=2)
    finished = float(ref[0][3].astype(bool).mean())
    print("%s: share of lanes finished by the first call %.3f" % (env, finished))
    if env != "network":
        assert .01 <= finished <= .99, finished
    assert ref[1][1] == 0
    r.check(k, ref)


# ---- 2. same draws as a tape ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", list(STEPS))
def test_a_tape_of_the_recorded_actions_reproduces_the_run(oracle_lib, env):
    k = STEPS[env]
    r = Run(oracle_lib, env, *random_tables(oracle_lib.OracleEnv(env)))
    r.rewind()
    out = r.e.run_controller(r.ctrl, k, layout="narrow")
    rows, st, done = rows_of(out, k), r.e.state.clone(), r.e._done.clone()
    tape = out["traj"][:k, 0, :N]                                    # the action plane is a tape as it stands
    r.rewind()
    taped = r.e.finish_episodes(k, actions=tape, layout="packed")
    assert np.array_equal(rows_of(taped, k), rows)
    assert torch.equal(r.e.state, st) and torch.equal(r.e._done, done) and r.e.invalid_action_count() == 0


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["rock", "tag"])
def test_results_do_not_depend_on_the_steps_per_launch(oracle_lib, env):
    """pomdp_fuse_max(3): eight steps as launches of 3 + 3 + 2, the node carried from one to the next"""
    from gym_pomdp_amd import _native
    L = _native.lib()
    k = 8
    r = Run(oracle_lib, env, *random_tables(oracle_lib.OracleEnv(env)))
    got = {}
    old = L.pomdp_fuse_max(0)
    try:
        for fuse in (old, 3):
            L.pomdp_fuse_max(fuse)
            r.rewind()
            rows = rows_of(r.e.run_controller(r.ctrl, k, layout="packed"), k)
            res = [rows, np_(r.e.state), np_(r.e._done), np_(r.ctrl.node)]
            r.rewind()
            stats = r.e.run_controller(r.ctrl, k)
            got[fuse] = res + [np_(stats.acc), np_(stats.cnt), np_(r.e.state), np_(r.ctrl.node)]
    finally:
        L.pomdp_fuse_max(old)
    for x, y in zip(got[old], got[3]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(got[3][0], r.reference(k)[0][0])


# ---- 4. table edges ------------------------------------------------------------------------------------------------------------
def test_a_controller_of_one_node(oracle_lib):
    o = oracle_lib.OracleEnv("tiger")
    r = Run(oracle_lib, "tiger", [0], np.zeros((1, o.n_obs), int), 0)
    r.check(6, r.reference(6, calls=2))


def test_the_largest_rocksample_controller(oracle_lib):
    """4096 nodes, 12 288 successors: sixteen rows of the action table and forty-eight of the successor table per staging
    thread.  Lanes start on nodes 0, 255, 256 and 4095, and lane 4 walks the chain 250 -> 251 -> ... across the first row's end
    (its nodes all check rock 0, which never ends an episode)."""
    o = oracle_lib.OracleEnv("rock")
    K, k = 4096, 16
    action, nxt, start = random_tables(o, nodes=K, seed=11)
    action[240:280] = 5
    nxt[240:280] = np.arange(241, 281)[:, None]
    start[:5] = [0, 255, 256, 4095, 250]
    r = Run(oracle_lib, "rock", action, nxt, start)
    ref = r.reference(k)
    assert ref[0][4][4] == 250 + k and not ref[0][3][4]               # the chain was walked to its sixteenth node, alive
    r.check(k, ref)


def test_the_largest_tag_controller(oracle_lib):
    """546 nodes x 30 observations = 16 380 successors, the last rows of the table in use: every node moves to node 545 on
    observation 29 (the agent stands on the opponent's cell), and node 545 keeps to itself"""
    o = oracle_lib.OracleEnv("tag")
    K, k = 546, 32
    action, nxt, start = random_tables(o, nodes=K, seed=13)
    action[:] = action % 4                                            # moves only: nobody tags, no episode ends early
    nxt[:, 29] = 545
    nxt[545] = 545
    start[start == 545] = 0
    r = Run(oracle_lib, "tag", action, nxt, start)
    ref = r.reference(k)
    assert (ref[0][4] == 545).any() and (ref[0][0] >> 8 & 0xFF == 29).any()
    r.check(k, ref)


# ---- 5. refused entries --------------------------------------------------------------------------------------------------------
def test_refused_entries_leave_their_lanes_alone_and_are_counted(oracle_lib):
    """validate=False: node 120 holds the action n_actions, every successor of node 121 is K, and lane 2 comes in on node K.
    Nodes 0 .. 119 move among themselves only, so no other lane meets any of it: those lanes equal the run of the clean
    controller."""
    o = oracle_lib.OracleEnv("rock")
    K, k = NODES, 8
    action, nxt, start = random_tables(o)
    nxt[:] = nxt % 120
    start[:] = start % 120
    clean = Run(oracle_lib, "rock", action.copy(), nxt.copy(), start.copy())
    clean.rewind()
    want = rows_of(clean.e.run_controller(clean.ctrl, k, layout="packed"), k)
    want_st, want_node = np_(clean.e.state), np_(clean.ctrl.node)
    action[120], action[121] = o.n_actions, 5                         # 121: check rock 0 — a step that stands, a lane that lives
    nxt[121] = K
    start[:3] = [120, 121, K]
    r = Run(oracle_lib, "rock", action, nxt, start, validate=False)
    ref = r.reference(k)
    packed, bad, st, done, node = ref[0][:5]
    assert bad == 3 * k
    assert (packed[:, 0] == o.n_actions).all() and (packed[:, 2] == 255).all()          # the byte, (ob, reward, done) = (0, 0, 0)
    assert (packed[:, 1] & 0xFF == 5).all() and not (packed[:, 1] >> 24).any()          # lane 1 steps
    assert np.array_equal(st[:, [0, 2]], r.st0[:, [0, 2]]) and node[:3].tolist() == [120, 121, K] and not done[:3].any()
    r.check(k, ref)
    r.rewind()
    got = rows_of(r.e.run_controller(r.ctrl, k, layout="packed"), k)
    assert r.e.invalid_action_count() == 3 * k
    assert np.array_equal(got[:, 3:], want[:, 3:])
    assert np.array_equal(np_(r.e.state)[:, 3:], want_st[:, 3:]) and np.array_equal(np_(r.ctrl.node)[3:], want_node[3:])


# ---- 6. a population in one call -----------------------------------------------------------------------------------------------
def test_a_population_runs_as_one_controller(oracle_lib):
    """concat of four controllers, lane i on controller i % 4: each lane's return is the one it gets when its controller runs
    alone on the same batch and seed, and so is every per-controller mean"""
    import gym_pomdp_amd as gpa
    M, k = 4, 16
    o = oracle_lib.OracleEnv("tiger")
    rng = np.random.RandomState(21)
    parts = [(rng.randint(0, o.n_actions, 8), rng.randint(0, 8, (8, o.n_obs))) for _ in range(M)]
    e = make_env("tiger")
    e.reset()
    st0 = e._state.clone()
    pop, offsets = gpa.Controller.concat(e, parts)
    lanes = np.arange(N)
    pop.start = np.asarray(offsets)[lanes % M]
    pop.reset_nodes()
    together = np_(e.run_controller(pop, k).ret_done)
    assert np.isfinite(together).any()
    for m, (action, nxt) in enumerate(parts):
        e._state.copy_(st0)
        e._done.zero_()
        e.call_counter = 1
        alone = np_(e.run_controller(gpa.Controller(e, action, nxt), k).ret_done)
        mine = lanes % M == m
        assert same_f64(together[mine], alone[mine]), m
        fin = mine & np.isfinite(alone)
        assert fin.any() and together[fin].mean() == alone[fin].mean(), m


# ---- 7. the episode loop end to end ----------------------------------------------------------------------------------------------
def test_finished_lanes_restart_on_their_start_node(oracle_lib):
    """Tiger, "listen twice, open the other door": run, ctrl.reset_nodes(where=env.done), env.reset(where=env.done), run again —
    the second run equals the restatement from the masked reset's state with the finished lanes back on node 0"""
    OPEN0, OPEN1, LISTEN = 0, 1, 2
    action = [LISTEN, LISTEN, LISTEN, OPEN1, OPEN0]
    nxt = [[1, 2, 0], [3, 0, 0], [0, 4, 0], [0, 0, 0], [0, 0, 0]]
    k = 16
    r = Run(oracle_lib, "tiger", action, nxt, 0)
    _, _, st, done, node = r.reference(k)[0][:5]
    fin = done.astype(bool)
    assert fin.any() and not fin.all()
    r.rewind()
    r.e.run_controller(r.ctrl, k)
    r.ctrl.reset_nodes(where=r.e.done)
    t = r.e.call_counter
    ob = r.e.reset(where=r.e.done)
    fresh = r.o.new_state(N)
    want_ob = r.o.batch_reset(fresh, SEED, LANE0, t, nthreads=r.nt)
    assert np.array_equal(np_(ob), np.where(fin, want_ob, -1)) and not bool(r.e.done.any())
    st, node, done = np.where(fin[None, :], fresh, st).astype(np.uint32), np.where(fin, 0, node), np.zeros(N, np.uint8)
    assert np.array_equal(np_(r.ctrl.node), node)
    packed, bad = cr.run(r.o, st, done, node, r.action, r.nxt, k, SEED, LANE0, t + 1, nthreads=r.nt)
    out = r.e.run_controller(r.ctrl, k, layout="packed")
    assert np.array_equal(rows_of(out, k), packed) and bad == 0 == r.e.invalid_action_count()
    assert np.array_equal(np_(r.e.state).view(np.uint32), st) and np.array_equal(np_(r.ctrl.node), node)
    assert np.array_equal(np_(r.e._done), done)
