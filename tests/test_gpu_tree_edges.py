"""The four tree searches on the GPU — pomdp_tree_search, pomdp_tree_search_preferred, pomdp_tree_search_resume with
pomdp_tree_advance, pomdp_tree_search_preferred_resume — where tests/test_gpu_key_edges.py and tests/test_gpu_env_params.py
took the older launches: at the edges of the Philox key and counter (K1, K2, K3 of tests/test_tree_edges_host.py, whose
tables, roots and coverage conditions this module shares), under the constructor parameters and action counts no search had
met (A = 65 and 100 among them), and at the argument edges the API accepts.  Every comparison is bit for bit against the
existing restatements: the ten keys of test_gpu_tree_search.py with float64 viewed as uint64, and after every advance the node
counts and the decoded trees.  Coverage is asserted on the restatement's side, on the very inputs the comparison ran on;
test_tree_edges_host.py shows on the oracle alone that each damaged coordinate changes these cases' simulations."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_keep_preferred_restatement as kp  # noqa: E402
import tree_keep_restatement as tk  # noqa: E402
import tree_search_preferred_restatement as tp  # noqa: E402
import test_gpu_preferred as gp  # noqa: E402
import test_gpu_tree_keep as gk  # noqa: E402
import test_gpu_tree_keep_preferred as gkp  # noqa: E402
import test_gpu_tree_search as gs  # noqa: E402
import test_gpu_tree_search_preferred as gsp  # noqa: E402
import test_tree_edges_host as th  # noqa: E402

pytestmark = pytest.mark.gpu
np_, u32, same = gs.np_, gs.u32, gs.same


# ---- one search of each kind against its restatement ------------------------------------------------------------------------
def uniform_search(env, kw, row, seed, lane_offset, t0, c=None, discount=None, what=None):
    """env.search() of a (R, W, S, D, P) row from test_gpu_tree_search.setup's roots -> (oracle, env, belief, restatement)"""
    R, W, S, D, P = row
    c = th.UCB[env] if c is None else c
    o, e, b = gs.setup(env, kw, R, lane_offset, P, t0=t0, seed=seed)
    assert np.array_equal(u32(e.state), th.uniform_roots(env, kw, R, lane_offset, seed)[1])     # the roots the host test counted on
    assert e._discount == th.discount_of(env)
    with np.errstate(over="ignore"):
        want = gs.restate(o, e, b, W, S, D, c, discount=discount, seed=seed)
    got = e.search(D, S, W, c, discount=discount, belief=b, diagnostics=True)
    assert e.call_counter == t0 + S * D
    same(got, want, what or (env, kw, row))
    return o, e, b, want


def preferred_search(env, kw, row, seed, lane_offset, t0, prior, c=None, what=None):
    """env.search(policy="preferred") from test_gpu_preferred.constructed's roots -> (oracle, env, got, restatement)"""
    R, W, S, D, P = row
    c = th.UCB[env] if c is None else c
    o, e, hist, b = gp.constructed(env, kw, R, th.PREP, P if P else 1, lane_offset, root_seed=th.ROOT_SEED, seed=seed)
    e.call_counter = t0
    want = gsp.restate(o, e, hist, b, W, S, D, c, prior, P)
    got = e.search(D, S, W, c, belief=b, diagnostics=True, policy="preferred", history=hist, prior_n=prior[0], prior_v=prior[1])
    assert e.call_counter == t0 + S * D
    same(got, want, what or (env, kw, row, prior))
    return o, e, got, want


def uniform_resume(env, kw, row, seed, lane_offset, t0, c=None, discount=None, steps=th.STEPS):
    """search_step(tree=) over `steps` real steps with C = 2 S + 1 (test_gpu_tree_keep.play: the ten keys per step, node counts
    and decoded trees per advance) -> (the oracle-side replay's searches, the largest kept tree per step)"""
    R, W, S, D, P = row
    with np.errstate(over="ignore"):
        seen = gk.play(env, kw, (R, W, lane_offset, S, D, 2 * S + 1, P, steps), seed=seed, t0=t0, c=th.UCB[env] if c is None else c,
                       discount=discount)
        res, kept = th.play_uniform(env, kw, seed, lane_offset, t0, row, 2 * S + 1, steps, c=c, discount=discount)
    assert kept == seen["kept_per_step"], (kept, seen)                       # the replay is the run the device was compared with
    return res, kept


def preferred_resume(env, kw, row, seed, lane_offset, t0, prior, steps=th.STEPS):
    """search_step(policy="preferred", history=, tree=[, belief=]) over `steps` real steps with C = 2 S + 1, as
    test_gpu_tree_keep_preferred.play compares it -> (the restatement's searches, the largest kept tree per step)"""
    R, W, S, D, P = row
    c, Cn = th.UCB[env], 2 * S + 1
    o, e, hist, b = gp.constructed(env, kw, R, th.PREP, P if P else 1, lane_offset, root_seed=th.ROOT_SEED, seed=seed)
    e.call_counter = t0
    tree = e.search_tree(W, Cn, D, policy="preferred", prior_n=prior[0], prior_v=prior[1])
    logn = kp.log_table(steps, S, o.n_actions, prior[0])
    trees, out, res, kept = None, None, [], []
    for step in range(steps):
        t = e.call_counter
        want = gkp.restate(o, e, hist, b, W, S, D, c, prior, P, trees, Cn, logn)
        ob, rew, done, info, got = e.search_step(D, S, W, c, belief=b, out=out, diagnostics=True, policy="preferred", history=hist,
                                                 tree=tree)
        out = got
        assert e.call_counter == t + S * D + 1 and tree.searches == step + 1
        same(got, want, (env, kw, row, prior, step))
        best, obs, dn = want["best"], np_(ob).reshape(R).astype(np.int32), np_(done).reshape(R).astype(bool)
        trees = tk.advance(want["trees"], W, best, obs, dn.astype(np.uint8))
        sizes = tk.n_nodes_of(trees)
        assert np.array_equal(np_(tree.n_nodes), sizes), (env, kw, row, step, np_(tree.n_nodes), sizes)
        for i in range(R * W):
            assert tk.same_canon(tree.to_host(i), tk.canon(trees[i])), (env, kw, row, prior, step, i)
        res.append(want)
        kept.append(int(sizes.max()))
    return res, kept


# ---- part 1: key and counter edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", th.U_SEARCH, ids=[th.u_id(c) for c in th.U_SEARCH])
def test_search_at_the_key_edges(case):
    ei, K, row = case
    env, kw = th.U_ENVS[ei]
    R, W, S, D, P = row
    seed, lane_offset, t0 = th.coords(K, R, W, S, D)
    _, e, _, want = uniform_search(env, kw, row, seed, lane_offset, t0)
    print(th.u_id(case), th.edge_coverage(want, K, R, W, S, D, P, seed, e.lane_offset * W, t0))
    host = th.run_uniform(env, kw, K, row)[0]                                # the host test's roots and particles are the device's
    assert all(host[k].tobytes() == want[k].tobytes() for k in th.TEN)


@pytest.mark.parametrize("case", th.P_SEARCH, ids=[th.p_id(c) for c in th.P_SEARCH])
def test_preferred_search_at_the_key_edges(case):
    ei, K, row, pi = case
    env, kw = th.P_ENVS[ei]
    R, W, S, D, P = row
    seed, lane_offset, t0 = th.coords(K, R, W, S, D)
    _, e, _, want = preferred_search(env, kw, row, seed, lane_offset, t0, th.PRIORS[pi])
    print(th.p_id(case), th.edge_coverage(want, K, R, W, S, D, P, seed, e.lane_offset * W, t0))
    assert want["stats"]["nan_prob"] == 0
    host = th.run_preferred(env, kw, K, row, th.PRIORS[pi])[0]               # the host test's roots are the device's
    assert all(host[k].tobytes() == want[k].tobytes() for k in th.TEN)


@pytest.mark.parametrize("case", th.U_RESUME, ids=[th.u_id(c) for c in th.U_RESUME])
def test_kept_trees_at_the_key_edges(case):
    ei, K, row = case
    env, kw = th.U_ENVS[ei]
    R, W, S, D, P = row
    seed, lane_offset, t0 = th.coords(K, R, W, S, D, resume=True)
    res, kept = uniform_resume(env, kw, row, seed, lane_offset, t0)
    print(th.u_id(case), th.resume_coverage(res, kept, K, row, seed, lane_offset * W, t0))


@pytest.mark.parametrize("case", th.P_RESUME, ids=[th.p_id(c) for c in th.P_RESUME])
def test_kept_preferred_trees_at_the_key_edges(case):
    ei, K, row, pi = case
    env, kw = th.P_ENVS[ei]
    R, W, S, D, P = row
    seed, lane_offset, t0 = th.coords(K, R, W, S, D, resume=True)
    res, kept = preferred_resume(env, kw, row, seed, lane_offset, t0, th.PRIORS[pi])
    print(th.p_id(case), th.resume_coverage(res, kept, K, row, seed, lane_offset * W, t0))
    assert sum(r["stats"]["kept_primed_reused"] for r in res[1:]) >= 1       # a kept, primed node was selected at above the carry
    host, host_kept = th.play_preferred(env, kw, seed, lane_offset, t0, row, 2 * S + 1, th.STEPS, th.PRIORS[pi])
    assert host_kept == kept and all(h[k].tobytes() == r[k].tobytes() for h, r in zip(host, res) for k in th.TEN)


# ---- part 3: env configurations ---------------------------------------------------------------------------------------------
CFG_ROWS = [th.ROW_A, th.ROW_B]
CFG_ROW_NAMES = ["6x4-S33-D10", "70x4-S2-D2-P4"]
U_GRID = [(i, j) for i in range(len(th.U_CONFIGS)) for j in range(2)]


@pytest.mark.parametrize("ci,ri", U_GRID, ids=["%s-%s" % (th.kwid(*th.U_CONFIGS[i]), CFG_ROW_NAMES[j]) for i, j in U_GRID])
def test_search_under_the_env_parameters(ci, ri):
    env, kw = th.U_CONFIGS[ci]
    R, W, S, D, P = CFG_ROWS[ri]
    _, e, _, want = uniform_search(env, kw, CFG_ROWS[ri], th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0)
    assert e.lane_offset * W == th.CFG_LANE0 and int(want["sim_steps"].max()) == D
    assert (want["n_nodes"] <= S + 1).all()


@pytest.mark.parametrize("env,kw,row,c", th.WIDE, ids=th.WIDE_IDS)
def test_search_with_more_than_64_actions(env, kw, row, c):
    """A = 65 and A = 100: the node pool's row pitch, the outputs' stride and the merge past one 64-bit mask, with trees that
    grow below the root"""
    R, W, S, D, P = row
    o, e, b, want = uniform_search(env, kw, row, th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0, c=c)
    assert o.n_actions > 64
    parts = None if b is None else u32(b.particles).copy()
    print(env, th.wide_coverage(o, u32(e.state).copy(), parts, want, row, c, e._discount))


P_ROWS = [th.ROW_A, th.ROW_A8]
P_ROW_NAMES = ["6x4-S33-D10", "12x4-S9-D10-P8"]
P_GRID = [(i, j, k) for i in range(len(th.P_CONFIGS)) for j in range(2) for k in (1, 0)]


@functools.lru_cache(maxsize=None)
def preferred_cfg(ci, ri, pi):
    """one configuration's preferred search, compared once -> the restatement's counters"""
    env, kw = th.P_CONFIGS[ci]
    R, W, S, D, P = P_ROWS[ri]
    prior = th.PRIORS[pi]
    _, e, got, want = preferred_search(env, kw, P_ROWS[ri], th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0, prior)
    if prior[0]:
        assert (want["root_prior_size"] >= 1).all()
        assert np.array_equal(np_(got["tree_visits"]).sum(axis=1), (want["sim_steps"] > 0).sum(axis=0) + prior[0] * want["root_prior_size"])
    return want["stats"]


@pytest.mark.parametrize("ci,ri,pi", P_GRID, ids=["%s-%s-%s" % (th.kwid(*th.P_CONFIGS[i]), P_ROW_NAMES[j], th.PRIOR_NAMES[k])
                                                  for i, j, k in P_GRID])
def test_preferred_search_under_the_env_parameters(ci, ri, pi):
    assert preferred_cfg(ci, ri, pi)["nan_prob"] == 0


def test_the_configurations_reach_the_policys_branches():
    """the restatement's counters over every preferred case above, on the inputs the comparisons ran on: Tag's per
    configuration, RockSample's over the union of its configurations"""
    print(th.branch_totals([th.P_CONFIGS[i] + (preferred_cfg(i, j, k),) for i, j, k in P_GRID]))


KEEP = [("uniform",) + c for c in th.U_KEEP] + [("preferred",) + c for c in th.P_KEEP]


@functools.lru_cache(maxsize=None)
def kept_cfg(i):
    kind, env, kw = KEEP[i]
    W = th.KEEP_ROW[1]
    if kind == "uniform":
        return uniform_resume(env, kw, th.KEEP_ROW, th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0)[1]
    return preferred_resume(env, kw, th.KEEP_ROW, th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0, th.PRIORS[2])[1]


@pytest.mark.parametrize("i", range(len(KEEP)), ids=["%s-%s" % (c[0], th.kwid(c[1], c[2])) for c in KEEP])
def test_kept_trees_under_the_env_parameters(i):
    print(KEEP[i], kept_cfg(i))


def test_some_configuration_keeps_a_subtree():
    assert max(max(kept_cfg(i)) for i in range(len(KEEP))) >= 2


# ---- part 4: argument edges -------------------------------------------------------------------------------------------------
ARG_ENVS = [("rock", {}), ("tag", {})]
ARG_ROW = (3, 4, 33, 10, 0)
C_MAX = 1.7976931348623157e308


@pytest.mark.parametrize("tree", [False, True], ids=["search", "tree"])
@pytest.mark.parametrize("discount", [1.0, 0.0])
@pytest.mark.parametrize("env,kw", ARG_ENVS, ids=["rock7-8", "tag"])
def test_a_discount_other_than_the_envs(env, kw, discount, tree):
    """discount = 1: the undiscounted sum; discount = 0: a return is its first reward, and 0 * acc stays out of the backup"""
    W = ARG_ROW[1]
    if tree:
        res, _ = uniform_resume(env, kw, ARG_ROW, th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0, discount=discount, steps=2)
        want = res[0]
    else:
        want = uniform_search(env, kw, ARG_ROW, th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0, discount=discount)[3]
    other = th.cfg_uniform(env, kw, ARG_ROW)[3]                              # the env's own discount: another result
    assert want["sim_ret"].tobytes() != other["sim_ret"].tobytes()


@pytest.mark.parametrize("tree", [False, True], ids=["search", "tree"])
@pytest.mark.parametrize("env,kw", ARG_ENVS, ids=["rock7-8", "tag"])
def test_the_largest_finite_ucb_c(env, kw, tree):
    """the bonus overflows to +inf wherever log(Nh) > 0: every visited action ties at +inf and the first wins"""
    W = ARG_ROW[1]
    if tree:
        res, _ = uniform_resume(env, kw, ARG_ROW, th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0, c=C_MAX, steps=2)
        want = res[0]
    else:
        want = uniform_search(env, kw, ARG_ROW, th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0, c=C_MAX)[3]
    assert np.isfinite(want["tree_q"]).all()


@pytest.mark.parametrize("prior_v", [1e300, -1e300])
@pytest.mark.parametrize("env,kw", ARG_ENVS, ids=["rock7-8", "tag"])
def test_the_largest_prior_count_and_huge_prior_values(env, kw, prior_v):
    """prior_n = 65535 with prior_v = +-1e300 and S = 2: the visit sums are the simulations plus prior_n * |P(0)| and stay
    below 2^31 at W = 4"""
    R, W, S, D = 3, 4, 2, 10
    _, e, got, want = preferred_search(env, kw, (R, W, S, D, 0), th.CFG_SEED, th.CFG_LANE0 // W, th.CFG_T0, (65535, prior_v))
    n_root = want["root_prior_size"]
    assert (n_root >= 1).all()
    sums = (want["sim_steps"] > 0).sum(axis=0) + 65535 * n_root
    assert np.array_equal(np_(got["tree_visits"]).astype(np.int64).sum(axis=1), sums)
    merged = np_(got["visits"]).astype(np.int64).sum(axis=1)
    assert np.array_equal(merged, sums.reshape(R, W).sum(axis=1)) and (merged < 1 << 31).all() and (merged > W * 65535).all()
    assert got["_logn"].numel() == S + 1 + e.action_space.n * 65535
