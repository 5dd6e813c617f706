"""POMCP's tree search on the GPU (pomdp_tree_search, BatchedEnv.search / search_step) against the contract's CPU restatement
(tests/tree_search_restatement.py), bit for bit: the trees' root statistics, their node counts, the three per-simulation
diagnostics and the merged q / visits / best / value.  The shapes are the smallest that reach each branch: R * W off the
wave and across a workgroup, S = 1 / 2 / 33, D = 0 / 1 / 2 / 10 (a rollout of more than four steps reads its second ROLLOUT
block), ucb_c = 0 / 1 / 100, true states and particles."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import particle_restatement as pr  # noqa: E402
import tree_search_restatement as ts  # noqa: E402

pytestmark = pytest.mark.gpu

ENV_IDS = {"rock": "Rock-v0", "stochrock": "StochasticRock-v0", "tag": "Tag-v0", "battleship": "Battleship-v0", "tiger": "Tiger-v0",
           "network": "Network-v0"}
ENVS = [("tiger", {}), ("rock", {}), ("rock", dict(board_size=15, num_rocks=15)), ("tag", {}), ("battleship", {}), ("network", {})]
ENV_NAMES = ["tiger", "rock7-8", "rock15-15", "tag", "battleship5x5", "network"]
# (R, W, lane_offset, S, D, ucb_c, P): every env runs every row
ROWS = [(3, 4, 0, 33, 10, 1.0, 0),          # 12 trees: a partial wave; deep trees, rollouts into their second ROLLOUT block
        (70, 4, 0, 2, 2, 100.0, 4),         # 280 trees: two workgroups, the second partial; from 4 particles
        (5, 1, 4, 1, 1, 0.0, 0),            # W = 1 at lane0 = 4; one simulation of one step
        (2, 16, 0, 33, 10, 0.0, 8),         # greedy, from 8 particles
        (3, 4, 0, 2, 0, 1.0, 0),            # D = 0: no simulation takes a step
        (70, 4, 0, 33, 2, 1.0, 0)]          # shallow and wide: many revisits of existing children
ROW_NAMES = ["3x4-S33-D10-c1", "70x4-S2-D2-c100-P4", "5x1@4-S1-D1-c0", "2x16-S33-D10-c0-P8", "3x4-S2-D0", "70x4-S33-D2-c1"]
SEED = 4242
KEYS = ("tree_visits", "tree_q", "n_nodes", "sim_ret", "sim_steps", "sim_tree_steps", "q", "visits", "best", "value")


def np_(t):
    return t.detach().cpu().numpy()


def u32(t):
    return np_(t).view(np.uint32)


def make(env, kw, n, **extra):
    import gym_pomdp_amd as gpa
    extra.setdefault("seed", SEED)
    extra.setdefault("auto_reset", False)
    return gpa.make(ENV_IDS[env], batch_size=n, **kw, **extra)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, what):
    for k in KEYS:
        g = np_(got[k]) if isinstance(got[k], torch.Tensor) else got[k]
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, (what, k, g.shape, g.dtype, want[k].shape, want[k].dtype)
        if not np.array_equal(bits(g), bits(want[k])):
            bad = np.argwhere(bits(g) != bits(want[k]))
            raise AssertionError("%s: %s differs at %d places, first %s: got %r, restatement %r"
                                 % (what, k, len(bad), bad[0], g[tuple(bad[0])], want[k][tuple(bad[0])]))


def setup(env, kw, R, lane_offset=0, P=0, warm=2, t0=None, seed=SEED):
    """an env `warm` synthetic steps into its episodes (so that roots differ in more than their hidden state), its belief
    when P > 0, and the oracle of the same configuration"""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv(env, **kw)
    e = make(env, kw, R, lane_offset=lane_offset, seed=seed)
    ob = e.reset()
    b = None
    if P:
        b = e.particle_belief(P)
        b.reset(ob)
    rs = np.random.RandomState(SEED)
    for _ in range(warm):
        a = torch.as_tensor(rs.randint(0, o.n_actions, R).astype(np.int32), device=e.device)
        ob, rew, done, _ = e.step(a)
        if b is not None:
            b.update(a, ob, rew, done)
    if t0 is not None:
        e.call_counter = t0
    return o, e, b


def restate(o, e, b, W, S, D, c, discount=None, seed=SEED):
    return ts.search(o, u32(e.state), e.batch_size, W, S, D, e._discount if discount is None else discount, c, seed,
                     e.lane_offset * W, e.call_counter, particles=None if b is None else u32(b.particles),
                     P=0 if b is None else b.n_particles)


GRID = [(i, j) for i in range(len(ENVS)) for j in range(len(ROWS))]


@pytest.mark.parametrize("ei,ri", GRID, ids=["%s-%s" % (ENV_NAMES[i], ROW_NAMES[j]) for i, j in GRID])
def test_search_matches_the_restatement(ei, ri):
    env, kw = ENVS[ei]
    R, W, lane_offset, S, D, c, P = ROWS[ri]
    o, e, b = setup(env, kw, R, lane_offset, P)
    want = restate(o, e, b, W, S, D, c)
    t0 = e.call_counter
    got = e.search(D, S, W, c, belief=b, diagnostics=True)
    assert e.call_counter == t0 + S * D
    same(got, want, (env, kw, ROWS[ri]))
    assert not [k for k, v in got.items() if not isinstance(v, torch.Tensor)]     # tensors only: no ctypes struct is kept
    if D == 0:
        assert (np_(got["best"]) == -1).all() and (np_(got["n_nodes"]) == 1).all()
    else:
        assert (np_(got["n_nodes"]) <= S + 1).all() and (np_(got["visits"]).sum(axis=1) <= W * S).all()


def test_a_shard_equals_its_roots_of_the_unsharded_search():
    """lane_offset != 0: roots 8 .. 13 of a 16-root search, run as a shard of 6 roots at lane_offset 8, give the same trees."""
    env, kw, W, S, D, c = "rock", {}, 4, 9, 6, 1.0
    o, e, _ = setup(env, kw, 16)
    t0 = e.call_counter
    full = e.search(D, S, W, c, diagnostics=True)
    sh = make(env, kw, 6, lane_offset=8)
    sh.reset()
    sh.set_state(e.state[:, 8:14])
    sh.call_counter = t0
    got = sh.search(D, S, W, c, diagnostics=True)
    for k in KEYS:
        f = np_(full[k])
        if k in ("q", "visits", "best", "value"):
            part = f[8:14]
        elif k.startswith("sim_"):
            part = f[:, 8 * W:14 * W]
        else:
            part = f[8 * W:14 * W]
        assert np.array_equal(bits(np_(got[k])), bits(part)), k
    same(got, ts.search(o, u32(sh.state), 6, W, S, D, sh._discount, c, SEED, 8 * W, t0), "shard")


@pytest.mark.parametrize("env", ["rock", "tag"])
def test_call_counter_carries_into_its_high_word_inside_a_search(env):
    """t0 = 2^32 - 3 with S = 3, D = 2: the steps run at t0 .. t0 + 5, the fourth with t_hi = 1"""
    o, e, _ = setup(env, {}, 9, t0=(1 << 32) - 3)
    want = restate(o, e, None, 4, 3, 2, 1.0)
    got = e.search(2, 3, 4, 1.0, diagnostics=True)
    assert e.call_counter == (1 << 32) + 3
    same(got, want, env)


def test_reusing_out_equals_fresh_buffers():
    o, e, b = setup("rock", {}, 7, P=8)
    t0 = e.call_counter
    first = e.search(5, 9, 4, 1.0, belief=b, diagnostics=True)
    keep = {k: np_(first[k]).copy() for k in KEYS}
    ws, logn = first["_workspace"].data_ptr(), first["_logn"].data_ptr()
    e.search(5, 9, 4, 50.0, belief=b, out=first, diagnostics=True)             # another search scribbles over every buffer
    e.call_counter = t0
    again = e.search(5, 9, 4, 1.0, belief=b, out=first, diagnostics=True)
    assert again is first and first["_logn"].data_ptr() == logn and first["_workspace"].data_ptr() == ws    # allocated once per out
    for k in KEYS:
        assert np.array_equal(bits(np_(again[k])), bits(keep[k])), k
    with pytest.raises(ValueError):
        e.search(5, 9, 8, 1.0, out=first)                                      # another shape


@pytest.mark.parametrize("P", [0, 8])
def test_search_step_is_search_then_step_then_belief_update(P):
    env, kw, R, W, S, D, c = "rock", {}, 9, 4, 9, 5, 2.0
    from oracle import oracle_lib as ol
    o, e, b = setup(env, kw, R, P=P)
    want = restate(o, e, b, W, S, D, c)
    real = u32(e.state).copy()
    ended = np_(e.done).astype(np.uint8)                                       # lanes the warm-up ended stay frozen: (0, 0, 1)
    t_step = e.call_counter + S * D
    ob, rew, done, info, got = e.search_step(D, S, W, c, belief=b, diagnostics=True)
    same(got, want, "search_step")
    assert (want["best"] >= 0).all()
    wob, wrew, wdone, bad = o.batch_step(real, want["best"], SEED, 0, t_step, auto_reset=False, done=ended)
    assert bad == 0 and e.call_counter == t_step + 1
    assert np.array_equal(np_(ob), wob) and np.array_equal(np_(rew), wrew) and np.array_equal(np_(done).astype(np.uint8), wdone)
    assert np.array_equal(u32(e.state), real)                                  # batch_step advanced `real` in place


def test_search_step_updates_the_belief_like_the_restatement():
    env, kw, R, W, S, D, c, P = "tag", {}, 6, 4, 5, 4, 2.0, 8
    o, e, b = setup(env, kw, R, P=P)
    parts = u32(b.particles).copy()
    tb = b.call_counter
    ob, rew, done, info, got = e.search_step(D, S, W, c, belief=b)
    a = np_(got["best"])
    want, nm = pr.update(o, parts, a, np_(ob), np_(rew).astype(o.reward_dtype), np_(done), False, R, P, b.seed, b.lane0, tb)
    assert np.array_equal(u32(b.particles), want)
    assert b.call_counter == tb + 1
    e2 = make(env, kw, R, auto_reset=True)
    e2.reset()
    with pytest.raises(ValueError):
        e2.search_step(D, S, W, c, belief=e2.particle_belief(P))
    with pytest.raises(TypeError):
        e2.search(D, S, W)                                                     # ucb_c has no default
