"""The preferred-policy search resumed from kept trees on the GPU (pomdp_tree_search_preferred_resume; search /
search_step(policy="preferred", history=, tree=) with a SearchTree built under policy="preferred") against the contract's CPU
restatement (tests/tree_keep_preferred_restatement.py), bit for bit: per real step the ten keys of test_gpu_tree_search.py,
and after each advance the node count and the decoded tree (to_host) of every tree.  The roots are the constructed ones of
test_gpu_tree_search_preferred.py; rows, priors, ucb_c and the REACHED table come from test_tree_keep_preferred_host.py, where
they were chosen on the oracle alone, and the branches are asserted here on the restatement's side, on the very inputs the
comparisons ran on.  A (env, row, priors) case is played once and shared (play())."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_keep_preferred_restatement as kp  # noqa: E402
import tree_keep_restatement as tk  # noqa: E402
import test_gpu_preferred as gp  # noqa: E402
from test_gpu_tree_search import KEYS, bits, same  # noqa: E402
from test_tree_keep_preferred_host import (ENVS, ENV_NAMES, PREP, ROOT_SEED, UCB, PRIORS, PRIOR_NAMES, ROWS, ROW_NAMES, REACHED,  # noqa: E402
                                           new_seen, observe, reached_of)

pytestmark = pytest.mark.gpu
np_, u32 = gp.np_, gp.u32
GRID = [(i, j, k) for i in range(len(ENVS)) for j in range(len(ROWS)) for k in ROWS[j][1]]


def inputs(e, hist, b, R, P):
    """what the restatement takes: the state columns and the roots' policy inputs (copies)"""
    belief, history, pob = gp.roots_of(e, hist)
    return u32(gp.columns_of(e, b)).reshape(-1, R * max(P, 1)).copy(), belief, history, pob


def restate(o, e, hist, b, W, S, D, c, prior, P, trees, Cn, logn):
    from oracle import oracle_lib as ol
    cols, belief, history, pob = inputs(e, hist, b, e.batch_size, P)
    return kp.search(o, cols, belief, history, pob, e.batch_size, W, S, D, e._discount, c, e._seed, e.lane_offset * W, e.call_counter,
                     trees=trees, C=Cn, logn=logn, P=P, prior_n=prior[0], prior_v=prior[1], nthreads=ol.max_threads())


@functools.lru_cache(maxsize=None)
def play(ei, ri, pi):
    """the row's real steps through search_step(policy="preferred", history=, tree=[, belief=]), each compared with the
    restatement -> what the restatement reached"""
    env, kw = ENVS[ei]
    (R, W, lane_offset, S, D, Cn, P, steps), _ = ROWS[ri]
    prior, c = PRIORS[pi], UCB[env]
    o, e, hist, b = gp.constructed(env, kw, R, PREP, P if P else 1, lane_offset, root_seed=ROOT_SEED)
    tree = e.search_tree(W, Cn, D, policy="preferred", prior_n=prior[0], prior_v=prior[1])
    assert tree.policy == "preferred" and (tree.prior_n, tree.prior_v) == prior
    assert (np_(tree.n_nodes) == 0).all() and tree.to_host(0) == {}
    logn, n = kp.log_table(steps, S, o.n_actions, prior[0]), R * W
    trees, seen, out, pws = None, new_seen(), None, None
    for step in range(steps):
        was_done = np_(e.done).astype(bool).reshape(R).copy()
        resumed = trees is not None and any(t is not None for t in trees)
        t0 = e.call_counter
        want = restate(o, e, hist, b, W, S, D, c, prior, P, trees, Cn, logn)
        ob, rew, done, info, got = e.search_step(D, S, W, c, belief=b, out=out, diagnostics=True, policy="preferred", history=hist,
                                                 tree=tree)
        out = got
        assert e.call_counter == t0 + S * D + 1 and tree.searches == step + 1
        assert tree._logn.numel() >= (step + 1) * S + o.n_actions * prior[0] + 1
        same(got, want, (ENV_NAMES[ei], ROW_NAMES[ri], PRIOR_NAMES[pi], step))
        assert not [k for k, v in got.items() if not isinstance(v, torch.Tensor)]     # the scratch is the tree's, not out's
        if env != "tag":
            assert pws in (None, tree._policy_workspace.data_ptr())          # allocated once
            pws = tree._policy_workspace.data_ptr()
        best, obs, dn = want["best"], np_(ob).reshape(R).astype(np.int32), np_(done).reshape(R).astype(bool)
        assert np.array_equal(np_(hist.prev_ob), obs)                         # the history followed the real step
        trees = tk.advance(want["trees"], W, best, obs, dn.astype(np.uint8))
        sizes = tk.n_nodes_of(trees)
        assert np.array_equal(np_(tree.n_nodes), sizes), (ENV_NAMES[ei], ROW_NAMES[ri], step, np_(tree.n_nodes), sizes)
        for i in range(n):
            assert tk.same_canon(tree.to_host(i), tk.canon(trees[i])), (ENV_NAMES[ei], ROW_NAMES[ri], PRIOR_NAMES[pi], step, i)
        observe(seen, want, resumed, trees, best, dn, was_done, R, W)
    return seen


@pytest.mark.parametrize("ei,ri,pi", GRID, ids=["%s-%s-%s" % (ENV_NAMES[i], ROW_NAMES[j], PRIOR_NAMES[k]) for i, j, k in GRID])
def test_search_step_with_a_preferred_tree_matches_the_restatement(ei, ri, pi):
    (R, W, lane_offset, S, D, Cn, P, steps), _ = ROWS[ri]
    seen = play(ei, ri, pi)
    print("%s %s %s: %r" % (ENV_NAMES[ei], ROW_NAMES[ri], PRIOR_NAMES[pi], seen))
    if ri == 0:
        assert seen["full"] == 0 and seen["kept"] >= 1, seen                  # C = 67 holds two searches' nodes and the kept ones
    if ri == 1:
        assert seen["full"] >= 1 and max(seen["sizes"]) == Cn, seen           # the pool did fill
    if ri == 3:
        assert seen["late"] >= 1, seen                                        # nodes made on a last step, primed by the next search
    if ri == 4 and PRIORS[pi] == (1, -20.0):
        assert seen["late"] >= 1 and seen["reused"] == 0, seen                # D = 1: every kept root arrives with Nh == 0
    if ri == 5:
        assert seen["kept"] == 0 and seen["sizes"] == [1] * steps and seen["full"] >= 1, seen
    if ri == 6:
        assert seen["kept"] == 0 and seen["nh"] == 0 and seen["late"] == 0, seen


@pytest.mark.parametrize("ei", range(len(ENVS)), ids=ENV_NAMES)
def test_the_rows_reach_every_branch(ei):
    """what REACHED says of this env, over all its rows and priors, on the inputs the comparisons ran on; under priors Tag's
    five-action root also passes Nh > S + A * prior_n at the first shape"""
    got = set()
    for i, ri, pi in GRID:
        if i == ei:
            got |= reached_of(play(ei, ri, pi))
    print(ENV_NAMES[ei], sorted(got))
    assert REACHED[ENV_NAMES[ei]] <= got, (REACHED[ENV_NAMES[ei]] - got)
    if ENVS[ei][0] == "tag":
        (R, W, lane_offset, S, D, Cn, P, steps), pis = ROWS[0]
        assert all(play(ei, 0, pi)["nh"] > S + 5 * PRIORS[pi][0] for pi in pis)


@pytest.mark.parametrize("pi", range(len(PRIORS)), ids=PRIOR_NAMES)
@pytest.mark.parametrize("ei", range(len(ENVS)), ids=ENV_NAMES)
def test_resume_from_empty_equals_the_preferred_search(ei, pi):
    """the anchor on the device: an empty preferred tree with C = S + 1 on the same counter — search(policy="preferred",
    prior_n, prior_v)'s ten keys, bit for bit; the priors come from the tree"""
    env, kw = ENVS[ei]
    R, W, S, D, prior = 3, 4, 33, 10, PRIORS[pi]
    o, e, hist, _ = gp.constructed(env, kw, R, PREP, 1, 0, root_seed=ROOT_SEED)
    t0 = e.call_counter
    want = e.search(D, S, W, UCB[env], diagnostics=True, policy="preferred", history=hist, prior_n=prior[0], prior_v=prior[1])
    e.call_counter = t0
    tree = e.search_tree(W, S + 1, D, policy="preferred", prior_n=prior[0], prior_v=prior[1])
    got = e.search(D, S, W, UCB[env], diagnostics=True, policy="preferred", history=hist, tree=tree)
    assert e.call_counter == t0 + S * D and tree._logn.numel() == S + 1 + o.n_actions * prior[0]
    for k in KEYS:
        assert np.array_equal(bits(np_(got[k])), bits(np_(want[k]))), (env, k)
    assert np.array_equal(np_(tree.n_nodes), np_(want["n_nodes"]))
    assert "_workspace" not in got and "_policy_workspace" not in got
    again = e.search(D, S, W, UCB[env], policy="preferred", history=hist, tree=tree, prior_n=prior[0], prior_v=prior[1])   # the tree's own: accepted
    assert (np_(again["visits"]).sum(axis=1) > np_(got["visits"]).sum(axis=1)).all()


@pytest.mark.parametrize("ei", range(len(ENVS)), ids=ENV_NAMES)
def test_a_resumed_search_writes_nothing_of_the_roots(ei):
    """a search from kept trees — the first search's trees advanced under a child that tree r * W holds, so that something is
    kept whatever the real step would have shown: the ten keys against the restatement, and the side statistics, the History
    tensors, the particles and the live state byte-identical afterwards"""
    env, kw = ENVS[ei]
    R, W, S, D, Cn, P, prior = 6, 4, 17, 8, 40, 8, (3, 5.0)
    o, e, hist, b = gp.constructed(env, kw, R, PREP, P, 0, root_seed=ROOT_SEED)
    tree = e.search_tree(W, Cn, D, policy="preferred", prior_n=prior[0], prior_v=prior[1])
    logn = kp.log_table(2, S, o.n_actions, prior[0])
    first = restate(o, e, hist, b, W, S, D, UCB[env], prior, P, None, Cn, logn)
    got = e.search(D, S, W, UCB[env], belief=b, diagnostics=True, policy="preferred", history=hist, tree=tree)
    same(got, first, (env, "first"))
    keys = [sorted(first["trees"][r * W].children[0]) for r in range(R)]
    act = np.array([k[0][0] if k else 0 for k in keys], np.int32)
    obs = np.array([k[0][1] if k else 0 for k in keys], np.int32)
    assert any(keys)
    tree.advance(act, obs)
    trees = tk.advance(first["trees"], W, act, obs)
    assert np.array_equal(np_(tree.n_nodes), tk.n_nodes_of(trees)) and int(tk.n_nodes_of(trees).max()) >= 1
    want = restate(o, e, hist, b, W, S, D, UCB[env], prior, P, trees, Cn, logn)
    before = inputs(e, hist, b, R, P)
    live = u32(e.state).copy()
    derived = (np_(hist.move_ok).copy(), np_(e._tracker.check_ok).copy()) if before[1] is not None else None
    t0 = e.call_counter
    got = e.search(D, S, W, UCB[env], belief=b, diagnostics=True, policy="preferred", history=hist, tree=tree)
    assert e.call_counter == t0 + S * D
    same(got, want, (env, "second"))
    after = inputs(e, hist, b, R, P)
    assert after[0].tobytes() == before[0].tobytes() and np.array_equal(u32(e.state), live)
    assert np.array_equal(after[3], before[3])
    for k in before[2]:
        assert after[2][k].tobytes() == before[2][k].tobytes(), k
    if before[1] is not None:
        for k in before[1]:
            assert after[1][k].tobytes() == before[1][k].tobytes(), k
        assert np.array_equal(np_(hist.move_ok), derived[0]) and np.array_equal(np_(e._tracker.check_ok), derived[1])


def test_the_interface_refusals():
    import gym_pomdp_amd as gpa
    e = gp.make("rock", {}, 4)
    hist = gpa.History(e, observation=e.reset())
    tree = e.search_tree(4, 19, 5, policy="preferred", prior_n=3, prior_v=5.0)
    with pytest.raises(ValueError, match="policy='preferred'"):
        e.search(5, 9, 4, 20.0, tree=tree)                                    # a preferred tree under the uniform search
    with pytest.raises(ValueError, match="differ"):
        e.search(5, 9, 4, 20.0, policy="preferred", history=hist, tree=tree, prior_n=2, prior_v=5.0)
    with pytest.raises(ValueError, match="differ"):
        e.search(5, 9, 4, 20.0, policy="preferred", history=hist, tree=tree, prior_n=3, prior_v=4.0)
    with pytest.raises(ValueError, match="does not resume.*search_tree"):
        e.search(5, 9, 4, 20.0, policy="preferred", history=hist, tree=e.search_tree(4, 19, 5))   # a tree grown without priors
    for bad in (dict(policy="preferred", prior_n=-1), dict(policy="preferred", prior_n=65536),
                dict(policy="preferred", prior_n=1, prior_v=float("nan")), dict(policy="preferred", prior_n=1, prior_v=float("inf")),
                dict(policy="greedy"), dict(prior_n=1)):                      # the last: priors go with policy="preferred"
        with pytest.raises(ValueError):
            e.search_tree(4, 19, 5, **bad)
    assert tree.searches == 0 and (np_(tree.n_nodes) == 0).all()              # no refused call touched the tree
    e.search(5, 9, 4, 20.0, policy="preferred", history=hist, tree=tree)
    assert tree.searches == 1
    # envs whose preferred search is the uniform one
    t = gp.make("tiger", {}, 4)
    t.reset()
    with pytest.raises(ValueError):
        t.search_tree(4, 19, 5, policy="preferred", prior_n=1)
    plain = gp.make("rock", dict(use_heuristic=False), 4)
    plain.reset()
    with pytest.raises(ValueError):
        plain.search_tree(4, 19, 5, policy="preferred", prior_n=1)
    assert plain.search_tree(4, 19, 5, policy="preferred").policy == "uniform"
    # auto_reset
    auto = gp.make("tag", {}, 4, auto_reset=True)
    auto.reset()
    with pytest.raises(ValueError, match="auto_reset"):
        auto.search_step(5, 9, 4, 10.0, policy="preferred", history=gpa.History(auto),
                         tree=auto.search_tree(4, 19, 5, policy="preferred", prior_n=1, prior_v=0.0))


def test_the_visit_budget_counts_the_priors_and_tells_the_caller_to_clear():
    import gym_pomdp_amd as gpa
    e = gp.make("tag", {}, 2)
    hist = gpa.History(e, observation=e.reset())
    W, S, pn = 4, 1000, 65535
    tree = e.search_tree(W, 3, 0, policy="preferred", prior_n=pn, prior_v=1.0)
    limit = 0x7FFFFFFF // W                                                   # (searches + 1) * S + A * prior_n may reach this
    tree.searches = (limit - 5 * pn) // S                                     # one more search passes it, by the priors' term alone:
    assert (tree.searches + 1) * S <= limit < (tree.searches + 1) * S + 5 * pn
    with pytest.raises(ValueError, match="clear"):
        e.search(0, S, W, 1.0, policy="preferred", history=hist, tree=tree)
    tree.clear()
    e.search(0, S, W, 1.0, policy="preferred", history=hist, tree=tree)      # D = 0: nothing is simulated
    assert tree.searches == 1 and tree._logn.numel() == S + 5 * pn + 1


def test_a_preferred_tree_without_priors_on_tiger_is_a_uniform_tree():
    import gym_pomdp_amd as gpa
    R, W, S, D, c = 5, 4, 9, 5, 10.0

    def run(**kw):
        t = gp.make("tiger", {}, R)
        t.reset()
        hist = gpa.History(t)
        tree = t.search_tree(W, 19, D, **kw)
        assert tree.policy == "uniform" and tree.prior_n == 0
        res = []
        for _ in range(3):
            ob, rew, done, info, got = t.search_step(D, S, W, c, diagnostics=True, policy="preferred", history=hist, tree=tree)
            res.append(({k: np_(got[k]).copy() for k in KEYS}, np_(tree.n_nodes).copy()))
        return res
    for (x, nx), (y, ny) in zip(run(), run(policy="preferred")):
        assert np.array_equal(nx, ny) and int(nx.max()) >= 1
        for k in KEYS:
            assert np.array_equal(bits(x[k]), bits(y[k])), k
