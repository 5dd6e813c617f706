"""Search trees kept between real steps on the GPU (pomdp_tree_search_resume, pomdp_tree_advance; search / search_step(tree=),
SearchTree) against the contract's CPU restatement (tests/tree_keep_restatement.py), bit for bit: per real step the ten keys
of test_gpu_tree_search.py, and after each advance the node count and the decoded tree (to_host) of every tree.  The shapes
are the smallest that reach each branch — kept subtrees, trees without the real step's child, ended lanes, Nh past S, a
full pool, particles, two workgroups, W = 1 at a lane offset, a pool of one node, D = 0 — and the test asserts on the
restatement's side that the branches were reached."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_keep_restatement as tk  # noqa: E402
import tree_search_restatement as ts  # noqa: E402
from test_gpu_tree_search import ENVS, ENV_NAMES, KEYS, SEED, bits, make, np_, same, setup, u32  # noqa: E402

pytestmark = pytest.mark.gpu

UCB = {"tiger": 10.0, "tag": 10.0, "network": 10.0, "rock": 20.0, "battleship": 5.0}
# (R, W, lane_offset, S, D, C, P, real steps)
ROWS = [(6, 4, 0, 33, 10, 67, 0, 4),        # kept subtrees, trees without the child, ended lanes, Nh > S; no pool fills
        (6, 4, 0, 33, 10, 34, 0, 4),        # the full-pool branch
        (2, 16, 0, 33, 10, 67, 8, 3),       # particles, W = 16
        (70, 4, 0, 2, 2, 5, 4, 3),          # two workgroups, the second partial
        (5, 1, 4, 1, 1, 3, 0, 3),           # W = 1 at a lane offset
        (3, 4, 0, 9, 5, 1, 0, 3),           # C = 1: a bandit at the root; every advance empties
        (3, 4, 0, 2, 0, 5, 0, 1)]           # D = 0: nothing simulated
ROW_NAMES = ["6x4-S33-D10-C67", "6x4-S33-D10-C34", "2x16-S33-D10-C67-P8", "70x4-S2-D2-C5-P4", "5x1@4-S1-D1-C3", "3x4-S9-D5-C1", "3x4-S2-D0"]
GRID = [(i, j) for i in range(len(ENVS)) for j in range(len(ROWS))]
# What the restatement reaches at the first shape, per env (seed 4242, two warm-up steps, the ucb_c above), found by running it
# and asserted below: "kept8" a kept tree of at least 8 nodes, "nomatch" a live lane's tree without the real step's child,
# "ended" a lane whose episode one of the four real steps ends, "frozen" a lane the warm-up had ended (searched and stepped all
# the same, its trees dropped every time).  RockSample's and Network's roots are wide (13 / 20 / 33 actions against 33
# simulations): their trees keep at most 7 nodes; of the six only Network has trees that miss the real step's child (4 of
# them), only Tag and BattleShip end an episode inside the four steps.  Every env's root passes Nh > S and keeps something.
REACHED = {"tiger": {"kept8", "frozen"}, "rock7-8": {"frozen"}, "rock15-15": set(), "tag": {"kept8", "ended"},
           "battleship5x5": {"kept8", "ended"}, "network": {"nomatch"}}


def play(env, kw, row, check_trees=True, seed=SEED, t0=None, c=None, discount=None):
    """`steps` real steps through search_step(tree=), each compared with the restatement -> what the restatement reached.
    seed, t0 (the call counter of the first search), c (ucb_c) and discount default to SEED, the counter after the warm-up,
    UCB[env] and the env's own"""
    R, W, lane_offset, S, D, Cn, P, steps = row
    c = UCB[env] if c is None else c
    o, e, b = setup(env, kw, R, lane_offset, P, t0=t0, seed=seed)
    gamma = e._discount if discount is None else discount
    tree = e.search_tree(W, Cn, D)
    assert (np_(tree.n_nodes) == 0).all() and tree.to_host(0) == {}
    trees, logn, n = None, ts.log_table(steps * S), R * W
    seen = dict(kept=0, nomatch=0, ended=0, frozen=0, nh=0, full=[], sizes=[])
    out = None
    for step in range(steps):
        was_done = np_(e.done).astype(bool).reshape(R).copy()
        t0 = e.call_counter
        want = tk.search(o, u32(e.state).copy(), R, W, S, D, gamma, c, seed, lane_offset * W, t0, trees=trees, C=Cn, logn=logn,
                         particles=None if b is None else u32(b.particles).copy(), P=P)
        ob, rew, done, info, got = e.search_step(D, S, W, c, discount=discount, belief=b, out=out, diagnostics=True, tree=tree)
        out = got
        assert e.call_counter == t0 + S * D + 1 and tree.searches == step + 1
        same(got, want, (env, kw, row, step))
        a, obs, dn = want["best"], np_(ob).reshape(R).astype(np.int32), np_(done).reshape(R).astype(bool)
        seen["nh"] = max(seen["nh"], max(t.Nh[0] for t in want["trees"]))
        seen["full"].append(int(want["full"].sum()))
        seen["sizes"].append(int(want["n_nodes"].max()))
        held = tk.n_nodes_of(want["trees"])
        trees = tk.advance(want["trees"], W, a, obs, dn.astype(np.uint8))
        sizes = tk.n_nodes_of(trees)
        assert np.array_equal(np_(tree.n_nodes), sizes), (env, row, step, np_(tree.n_nodes), sizes)
        assert (sizes < np.maximum(held, 1)).all()                            # the old root never survives
        if check_trees:
            for i in range(n):
                assert tk.same_canon(tree.to_host(i), tk.canon(trees[i])), (env, row, step, i)
        live = ~dn & (a >= 0)
        seen["kept"] = max(seen["kept"], int(sizes.max()))
        seen.setdefault("kept_per_step", []).append(int(sizes.max()))
        seen["nomatch"] += int((sizes.reshape(R, W)[live] == 0).sum())
        seen["ended"] += int((dn & ~was_done).sum())
        seen["frozen"] += int(was_done.sum())
        assert (sizes.reshape(R, W)[~live] == 0).all()                        # ended lanes and best == -1 lanes end up empty
    return seen


@pytest.mark.parametrize("ei,ri", GRID, ids=["%s-%s" % (ENV_NAMES[i], ROW_NAMES[j]) for i, j in GRID])
def test_search_step_with_a_tree_matches_the_restatement(ei, ri):
    env, kw = ENVS[ei]
    row = ROWS[ri]
    R, W, lane_offset, S, D, Cn, P, steps = row
    seen = play(env, kw, row)
    print("%s %s: %r" % (ENV_NAMES[ei], ROW_NAMES[ri], seen))
    if ri == 0:
        reached = REACHED[ENV_NAMES[ei]]
        assert seen["nh"] > S, seen                                           # a root's Nh indexes the log table past entry S
        assert not any(seen["full"]), seen                                    # C = 67 holds two searches' nodes and the kept ones
        assert ("kept8" not in reached) or seen["kept"] >= 8, seen
        assert ("nomatch" not in reached) or seen["nomatch"] >= 1, seen
        assert ("ended" not in reached) or seen["ended"] >= 1, seen
        assert ("frozen" not in reached) or seen["frozen"] >= 1, seen
        assert seen["kept"] >= 1, seen                                        # every env keeps something
    if ri == 1:
        assert sum(seen["full"]) >= 1 and max(seen["sizes"]) == Cn, seen      # the pool did fill
    if ri == 5:
        assert seen["kept"] == 0 and seen["sizes"] == [1] * steps, seen
    if ri == 6:
        assert seen["kept"] == 0 and seen["nh"] == 0, seen


def test_every_branch_is_reached_by_some_env():
    """kept >= 8 nodes, a tree without the child, an ended lane, a frozen lane: each is asserted for at least one env of the
    first shape"""
    assert set.union(*REACHED.values()) == {"kept8", "nomatch", "ended", "frozen"}


@pytest.mark.parametrize("ei", range(len(ENVS)), ids=ENV_NAMES)
def test_resume_from_empty_equals_search(ei):
    """the anchor: C = S + 1 from empty trees on the same counter — env.search()'s ten keys, bit for bit"""
    env, kw = ENVS[ei]
    R, W, S, D = 3, 4, 33, 10
    o, e, _ = setup(env, kw, R)
    t0 = e.call_counter
    want = e.search(D, S, W, UCB[env], diagnostics=True)
    e.call_counter = t0
    tree = e.search_tree(W, S + 1, D)
    got = e.search(D, S, W, UCB[env], diagnostics=True, tree=tree)
    assert e.call_counter == t0 + S * D and tree._logn.numel() == S + 1
    for k in KEYS:
        assert np.array_equal(bits(np_(got[k])), bits(np_(want[k]))), (env, k)
    assert np.array_equal(np_(tree.n_nodes), np_(want["n_nodes"]))
    assert "_workspace" not in got and not [k for k, v in got.items() if not isinstance(v, torch.Tensor)]


def test_a_shard_equals_its_roots_of_the_unsharded_run():
    """roots 8 .. 13 of 16, run as a shard of 6 roots at lane_offset 8, over two real steps: the same results and the same trees"""
    env, kw, W, S, D, c, Cn = "tag", {}, 4, 9, 6, 10.0, 19
    o, e, _ = setup(env, kw, 16)
    sh = make(env, kw, 6, lane_offset=8)
    sh.reset()
    sh.set_state(e.state[:, 8:14])
    sh.call_counter = e.call_counter
    tf, tsh = e.search_tree(W, Cn, D), sh.search_tree(W, Cn, D)
    for step in range(2):
        full = e.search(D, S, W, c, diagnostics=True, tree=tf)
        got = sh.search(D, S, W, c, diagnostics=True, tree=tsh)
        for k in KEYS:
            f = np_(full[k])
            part = f[8:14] if k in ("q", "visits", "best", "value") else f[:, 8 * W:14 * W] if k.startswith("sim_") else f[8 * W:14 * W]
            assert np.array_equal(bits(np_(got[k])), bits(part)), (step, k)
        # the same real step on both: the unsharded run's best action and a made-up observation per root that some trees hold
        a = full["best"]
        ob = torch.zeros(16, dtype=torch.int32, device=e.device)
        for r in range(16):
            kids = [p[0][1] for p in tf.to_host(r * W) if len(p) == 1 and p[0][0] == int(a[r])]
            ob[r] = kids[0] if kids else 0
        tf.advance(a, ob)
        tsh.advance(a[8:14], ob[8:14])
        assert np.array_equal(np_(tsh.n_nodes), np_(tf.n_nodes)[8 * W:14 * W])
        if step == 0:
            assert int(np_(tsh.n_nodes).max()) >= 2                           # something was kept
        for i in range(6 * W):
            assert tk.same_canon(tsh.to_host(i), tf.to_host(8 * W + i)), (step, i)


def test_clear_empties_exactly_the_masked_lanes():
    env, kw, R, W, S, D = "tiger", {}, 5, 4, 9, 5
    o, e, _ = setup(env, kw, R)
    tree = e.search_tree(W, sims_per_tree=S, depth=D)
    assert tree.node_capacity == 2 * S + 1
    e.search(D, S, W, 10.0, tree=tree)
    before = np_(tree.n_nodes).copy()
    assert (before >= 2).all()
    mask = torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8, device=e.device)
    tree.clear(where=mask)
    after = np_(tree.n_nodes).reshape(R, W)
    assert (after[[1, 4]] == 0).all() and np.array_equal(after[[0, 2, 3]], before.reshape(R, W)[[0, 2, 3]])
    assert tree.to_host(1 * W) == {} and len(tree.to_host(0)) == before[0] and tree.searches == 1
    tree.clear()
    assert (np_(tree.n_nodes) == 0).all() and tree.searches == 0
    with pytest.raises(ValueError):
        e.search_tree(W)                                                       # neither node_capacity nor sims_per_tree


def test_reusing_out_equals_fresh_buffers():
    env, kw, R, W, S, D, c, Cn = "rock", {}, 7, 4, 9, 5, 20.0, 19

    def run(reuse):
        o, e, b = setup(env, kw, R, P=8)
        tree, out, res = e.search_tree(W, Cn, D), None, []
        for step in range(3):
            ob, rew, done, info, got = e.search_step(D, S, W, c, belief=b, out=out if reuse else None, diagnostics=True, tree=tree)
            if reuse:
                assert out is None or got is out
                out = got
            res.append(({k: np_(got[k]).copy() for k in KEYS}, np_(tree.n_nodes).copy()))
        return res
    for (x, nx), (y, ny) in zip(run(False), run(True)):
        assert np.array_equal(nx, ny)
        for k in KEYS:
            assert np.array_equal(bits(x[k]), bits(y[k])), k


def test_a_tree_of_another_shape_is_refused():
    e = make("tiger", {}, 4)
    e.reset()
    tree = e.search_tree(4, 19, 5)
    e.search(5, 9, 4, 10.0, tree=tree)
    with pytest.raises(ValueError):
        e.search(5, 9, 2, 10.0, tree=tree)                                    # another W
    with pytest.raises(ValueError):
        e.search(6, 9, 4, 10.0, tree=tree)                                    # another D
    other = make("tag", {}, 4)
    other.reset()
    with pytest.raises(ValueError):
        other.search(5, 9, 4, 10.0, tree=tree)                                # another env
    wider = make("tiger", {}, 8)
    wider.reset()
    with pytest.raises(ValueError):
        wider.search(5, 9, 4, 10.0, tree=tree)                                # another batch
    auto = make("tiger", {}, 4, auto_reset=True)
    auto.reset()
    with pytest.raises(ValueError):
        auto.search_step(5, 9, 4, 10.0, tree=auto.search_tree(4, 19, 5))      # a restarted lane's tree would be the old episode's


def test_the_visit_budget_tells_the_caller_to_clear():
    e = make("tiger", {}, 2)
    e.reset()
    tree = e.search_tree(4, 3, 0)
    tree.searches = (0x7FFFFFFF // 4) // 1000                                 # W * searches * S is about to pass 2^31 - 1
    with pytest.raises(ValueError, match="clear"):
        e.search(0, 1000, 4, 1.0, tree=tree)
    tree.clear()
    e.search(0, 1000, 4, 1.0, tree=tree)                                      # D = 0: nothing is simulated


def test_the_preferred_policy_search_does_not_resume_yet():
    import gym_pomdp_amd as gpa
    e = make("rock", {}, 4, use_heuristic=True)
    hist = gpa.History(e, observation=e.reset())
    tree = e.search_tree(4, 19, 5)
    with pytest.raises(ValueError, match="does not resume"):
        e.search(5, 9, 4, 20.0, policy="preferred", history=hist, tree=tree)
    with pytest.raises(ValueError, match="does not resume"):
        e.search_step(5, 9, 4, 20.0, policy="preferred", history=hist, tree=tree)
    t = make("tiger", {}, 4)
    t.reset()
    got = t.search(5, 9, 4, 10.0, policy="preferred", history=gpa.History(t), tree=t.search_tree(4, 19, 5))     # forwards to the uniform search
    assert (np_(got["visits"]).sum(axis=1) == 4 * 9).all()
