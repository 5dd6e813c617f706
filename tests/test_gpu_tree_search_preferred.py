"""The preferred-policy tree search on the GPU (pomdp_tree_search_preferred; search / search_step(policy="preferred", history=,
prior_n=, prior_v=)) against the contract's CPU restatement (tests/tree_search_preferred_restatement.py), bit for bit on the
ten keys test_gpu_tree_search.py compares.  The roots are prepared ones (reset() plus six real heuristic-policy steps) with
the statistics of rr.construct_roots written over them, so that the simulations reach every branch of the policy and of the
copy-on-first-touch workspace; the restatement's counters, on the very inputs it ran, say so (test_the_rows_reach_every_branch).
A (env, row, priors) case is restated once and shared (case())."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preferred_rollout_restatement as rr  # noqa: E402
import tree_search_preferred_restatement as tp  # noqa: E402
import test_gpu_preferred as gp  # noqa: E402
from test_gpu_tree_search import KEYS, bits, same  # noqa: E402

pytestmark = pytest.mark.gpu
np_, u32 = gp.np_, gp.u32

ENVS = [("rock", {}), ("rock", dict(board_size=15, num_rocks=15)), ("stochrock", {}), ("tag", {})]
ENV_NAMES = ["rock7-8", "rock15-15", "stochrock", "tag"]
PREP = 6
ROOT_SEED = 1                                                  # rr.construct_roots' seed, chosen on the CPU (ROWS' counters below)
PRIORS = [(0, 0.0), (3, 5.0), (1, -20.0)]
PRIOR_NAMES = ["no-priors", "n3-v5", "n1-v-20"]
# (R, W, lane_offset, S, D, ucb_c, P, t0 or None, the priors the row runs under)
ROWS = [(3, 4, 0, 33, 10, 1.0, 0, None, (0, 1, 2)),         # a partial wave; a second ROLLOUT block; repeated CHECKs inside and across simulations
        (70, 4, 0, 2, 2, 100.0, 4, None, (0, 1, 2)),        # two workgroups, the second partial; particles (node 0's priors from a particle)
        (5, 1, 4, 1, 1, 0.0, 0, None, (0, 1, 2)),           # lane0 = 4; the node is created on the last step: it stays without priors
        (2, 16, 0, 33, 10, 0.0, 8, None, (0, 1, 2)),        # greedy selection over priors
        (3, 4, 0, 2, 0, 1.0, 0, None, (0, 1)),              # D == 0: no priors whatever prior_n says; best == -1
        (70, 4, 0, 33, 2, 1.0, 0, None, (0, 1, 2)),         # revisits of existing children, with Nh over S
        (3, 4, 0, 33, 10, 1.0, 0, (1 << 32) - 3, (0,)),     # the call counter carries into its high word inside the search
        (6, 4, 8, 9, 6, 1.0, 0, None, (0, 1))]              # a shard at lane_offset 8 (the restatement's lanes are the unsharded search's)
ROW_NAMES = ["3x4-S33-D10-c1", "70x4-S2-D2-c100-P4", "5x1@4-S1-D1-c0", "2x16-S33-D10-c0-P8", "3x4-S2-D0", "70x4-S33-D2-c1",
             "3x4-S33-D10-t0-carry", "6x4@8-S9-D6"]
GRID = [(i, j, k) for i in range(len(ENVS)) for j in range(len(ROWS)) for k in ROWS[j][8]]


def inputs(e, hist, b, R, P):
    """what the restatement takes: the state columns and the roots' policy inputs (copies)"""
    belief, history, pob = gp.roots_of(e, hist)
    return u32(gp.columns_of(e, b)).reshape(-1, R * max(P, 1)).copy(), belief, history, pob


def restate(o, e, hist, b, W, S, D, c, prior, P):
    cols, belief, history, pob = inputs(e, hist, b, e.batch_size, P)
    return tp.search(o, cols, belief, history, pob, e.batch_size, W, S, D, e._discount, c, e._seed, e.lane_offset * W,
                     e.call_counter, P=P, prior_n=prior[0], prior_v=prior[1])


@functools.lru_cache(maxsize=None)
def case(ei, ri, pi):
    """the env at constructed roots, its History and belief, and the restatement of the search from there — computed once"""
    env, kw = ENVS[ei]
    R, W, lane_offset, S, D, c, P, t0, _ = ROWS[ri]
    o, e, hist, b = gp.constructed(env, kw, R, PREP, P if P else 1, lane_offset, root_seed=ROOT_SEED)
    if t0 is not None:
        e.call_counter = t0
    return o, e, hist, b, e.call_counter, restate(o, e, hist, b, W, S, D, c, PRIORS[pi], P)


@pytest.mark.parametrize("ei,ri,pi", GRID, ids=["%s-%s-%s" % (ENV_NAMES[i], ROW_NAMES[j], PRIOR_NAMES[k]) for i, j, k in GRID])
def test_search_matches_the_restatement(ei, ri, pi):
    R, W, lane_offset, S, D, c, P, _, _ = ROWS[ri]
    o, e, hist, b, t0, want = case(ei, ri, pi)
    before = inputs(e, hist, b, R, P)
    live = u32(e.state).copy()
    derived = (np_(hist.move_ok).copy(), np_(e._tracker.check_ok).copy()) if before[1] is not None else None
    e.call_counter = t0
    got = e.search(D, S, W, c, belief=b, diagnostics=True, policy="preferred", history=hist, prior_n=PRIORS[pi][0],
                   prior_v=PRIORS[pi][1])
    assert e.call_counter == t0 + S * D
    same(got, want, (ENV_NAMES[ei], ROW_NAMES[ri], PRIOR_NAMES[pi]))
    assert not [k for k, v in got.items() if not isinstance(v, torch.Tensor)]     # tensors only: no ctypes struct is kept
    if D == 0:
        assert (np_(got["best"]) == -1).all() and (np_(got["n_nodes"]) == 1).all() and (np_(got["tree_visits"]) == 0).all()
    elif PRIORS[pi][0]:
        n_root = want["root_prior_size"]
        assert (n_root >= 1).all()
        assert np.array_equal(np_(got["tree_visits"]).sum(axis=1), (want["sim_steps"] > 0).sum(axis=0) + PRIORS[pi][0] * n_root)
    # the side statistics, the History tensors, the particles and the live state are byte-identical after the search
    after = inputs(e, hist, b, R, P)
    assert after[0].tobytes() == before[0].tobytes() and np.array_equal(u32(e.state), live)
    assert np.array_equal(after[3], before[3])
    for k in before[2]:
        assert after[2][k].tobytes() == before[2][k].tobytes(), k
    if before[1] is not None:
        for k in before[1]:
            assert after[1][k].tobytes() == before[1][k].tobytes(), k
        assert np.array_equal(np_(hist.move_ok), derived[0]) and np.array_equal(np_(e._tracker.check_ok), derived[1])


@pytest.mark.parametrize("ei", range(len(ENVS)), ids=ENV_NAMES)
def test_the_rows_reach_every_branch(ei):
    """the restatement's counters over all rows of one env, on the inputs the comparisons ran on"""
    total = {c: 0 for c in tp.COUNTERS}
    with_priors = 0
    for i, ri, pi in GRID:
        if i != ei:
            continue
        stats = case(ei, ri, pi)[5]["stats"]
        for c in total:
            total[c] += stats[c]
        if PRIORS[pi][0]:
            with_priors += stats["prior_from_fallback"]
    print(ENV_NAMES[ei], total, "prior_from_fallback under priors:", with_priors)
    assert total["nan_prob"] == 0
    if ENVS[ei][0] == "tag":
        assert total["corner_tag"] >= 1 and total["empty_history_all_five"] >= 1
        return
    for c in ("repeat_check", "recheck_across_sims", "fallback", "sample_rule", "all_bad_east", "check_ok_cleared",
              "move_bit_up", "move_bit_down", "sample_bit_up", "sample_bit_down"):
        assert total[c] >= 1, (c, total)
    assert with_priors >= 1, total


def test_a_shard_equals_its_roots_of_the_unsharded_search():
    """roots 8 .. 13 of a 16-root search, run as a shard of 6 roots at lane_offset 8 with the same policy inputs"""
    import gym_pomdp_amd as gpa
    env, kw = ENVS[0]
    R, W, lane_offset, S, D, c, P, _, _ = ROWS[7]
    o, e, hist, _ = gp.constructed(env, kw, 16, PREP, 1, 0, root_seed=ROOT_SEED)
    t0 = e.call_counter
    full = e.search(D, S, W, c, diagnostics=True, policy="preferred", history=hist, prior_n=3, prior_v=5.0)
    lo, hi = lane_offset, lane_offset + R
    belief, history, pob = gp.roots_of(e, hist)
    sh = gp.make(env, kw, R, lane_offset=lane_offset)
    sh.reset()
    sh.set_state(e.state[:, lo:hi])
    h = gpa.History(sh)
    rr.put_roots(sh, h, {k: v[:, lo:hi] for k, v in belief.items()}, {k: v[..., lo:hi] for k, v in history.items()}, pob[lo:hi])
    sh.call_counter = t0
    got = sh.search(D, S, W, c, diagnostics=True, policy="preferred", history=h, prior_n=3, prior_v=5.0)
    for k in KEYS:
        f = np_(full[k])
        part = f[lo:hi] if k in ("q", "visits", "best", "value") else f[:, lo * W:hi * W] if k.startswith("sim_") else f[lo * W:hi * W]
        assert np.array_equal(bits(np_(got[k])), bits(part)), k


@pytest.mark.parametrize("env,kw", [("tiger", {}), ("battleship", {}), ("network", {}), ("rock", dict(use_heuristic=False))],
                         ids=["tiger", "battleship", "network", "rock-without-use_heuristic"])
def test_envs_without_a_policy_run_the_uniform_search(env, kw):
    import gym_pomdp_amd as gpa
    R, W, S, D, c = 9, 4, 9, 5, 1.0
    e = gp.make(env, kw, R)
    e.reset()
    hist = gpa.History(e)
    for _ in range(2):
        e.step(e.synthetic_actions())
    t0 = e.call_counter
    u = e.search(D, S, W, c, diagnostics=True)
    e.call_counter = t0
    p = e.search(D, S, W, c, diagnostics=True, policy="preferred", history=hist)
    for k in KEYS:
        assert np_(u[k]).tobytes() == np_(p[k]).tobytes(), (env, k)
    assert int(np_(u["sim_steps"]).max()) >= 1
    with pytest.raises(ValueError):
        e.search(D, S, W, c, policy="preferred", history=hist, prior_n=1)
    with pytest.raises(ValueError):
        e.search(D, S, W, c, prior_n=1)                                     # priors go with the preferred policy
    with pytest.raises(ValueError):
        e.search(D, S, W, c, history=hist)                                  # history= goes with policy="preferred"


def test_refusals():
    import gym_pomdp_amd as gpa
    e = gp.make("rock", {}, 8)
    e.reset()
    hist = gpa.History(e)
    other = gp.make("rock", {}, 8)
    other.reset()
    for bad in (dict(policy="preferred"), dict(policy="preferred", history=gpa.History(e, max_size=5)),
                dict(policy="preferred", history=gpa.History(other)), dict(policy="greedy", history=hist),
                dict(policy="preferred", history=hist, prior_n=-1), dict(policy="preferred", history=hist, prior_n=65536),
                dict(policy="preferred", history=hist, prior_n=1, prior_v=float("nan")),
                dict(policy="preferred", history=hist, prior_n=1, prior_v=float("inf"))):
        with pytest.raises(ValueError):
            e.search(4, 4, 4, 1.0, **bad)
    auto = gp.make("rock", {}, 8, auto_reset=True)
    auto.reset()
    with pytest.raises(ValueError):
        auto.search_step(4, 4, 4, 1.0, policy="preferred", history=gpa.History(auto))


@pytest.mark.parametrize("ei", [0, 3], ids=["rock7-8", "tag"])
def test_search_step_is_search_step_append_and_belief_update(ei):
    """search_step(policy="preferred", history=, belief=) over three real steps against the restatements of its parts: the
    search (tp.search), the step (the oracle's batch_step), the history append and the side statistics
    (HistorySums.append / Belief.update), and the particle update (particle_restatement.update)"""
    import particle_restatement as pr
    from oracle import oracle_lib as ol
    env, kw = ENVS[ei]
    R, W, S, D, c, P, prior = 9, 4, 9, 5, 2.0, 8, (3, 5.0)
    o, e, hist, b = gp.constructed(env, kw, R, PREP, P, 0, root_seed=ROOT_SEED)
    frozen = np_(e.done).astype(np.uint8)
    for _ in range(3):
        cols, belief, history, pob = inputs(e, hist, b, R, P)
        want = restate(o, e, hist, b, W, S, D, c, prior, P)
        real = u32(e.state).copy()
        t_step, tb = e.call_counter + S * D, b.call_counter
        ob, rew, done, info, got = e.search_step(D, S, W, c, belief=b, diagnostics=True, policy="preferred", history=hist,
                                                 prior_n=prior[0], prior_v=prior[1])
        same(got, want, "search_step")
        best = want["best"]
        wob, wrew, wdone, _ = o.batch_step(real, best, e._seed, 0, t_step, auto_reset=False, done=frozen.copy())
        assert e.call_counter == t_step + 1 and np.array_equal(u32(e.state), real)
        assert np.array_equal(np_(ob), wob) and np.array_equal(np_(rew), wrew) and np.array_equal(np_(done).astype(np.uint8), wdone)
        bel, hs, p = rr.expand(o, belief, history, pob, R, 1)
        live = frozen == 0                                               # a lane that had ended stays as it is (best is -1 or ignored)
        if bel is not None:
            bel.update(real, np.where(live, best, 0).astype(np.int32), np.where(live, wob, 0).astype(np.int32),
                       np.where(live, wdone, 1).astype(np.uint8), auto_reset=False)
        belief1, history1, pob1 = gp.roots_of(e, hist)
        hs.append(p, best.astype(np.int32), wob.astype(np.int32), wdone, auto_reset=False)
        assert np.array_equal(pob1, wob)
        for k in ("size", "last_action", "last_ob") + (("total_sample", "total_move") if bel is not None else ()):
            assert np.array_equal(history1[k], getattr(hs, k)), k
        if bel is not None:
            for k, _ in ol.Belief.FIELDS:
                assert belief1[k].tobytes() == getattr(bel, k).tobytes(), k
        wparts, _ = pr.update(o, cols, best, wob, wrew.astype(o.reward_dtype), wdone, False, R, P, b.seed, b.lane0, tb)
        assert np.array_equal(u32(b.particles), wparts) and b.call_counter == tb + 1
        frozen = wdone.astype(np.uint8) | frozen


def test_reusing_out_equals_fresh_buffers_across_prior_counts():
    env, kw = ENVS[0]
    R, W, S, D, c, P = 7, 4, 9, 5, 1.0, 8
    o, e, hist, b = gp.constructed(env, kw, R, PREP, P, 0, root_seed=ROOT_SEED)
    t0 = e.call_counter
    kwargs = dict(belief=b, diagnostics=True, policy="preferred", history=hist)
    first = e.search(D, S, W, c, prior_n=3, prior_v=5.0, **kwargs)
    keep = {k: np_(first[k]).copy() for k in KEYS}
    n_log = first["_logn"].numel()
    assert n_log == S + 1 + 3 * e.action_space.n
    ws, pws = first["_workspace"].data_ptr(), first["_policy_workspace"].data_ptr()
    e.call_counter = t0
    plain = {k: np_(v).copy() for k, v in e.search(D, S, W, c, **kwargs).items() if k in KEYS}
    e.search(D, S, W, 50.0, out=first, prior_n=0, **kwargs)                    # scribbles over every buffer; the log table shrinks
    assert first["_logn"].numel() == S + 1
    e.call_counter = t0
    again = e.search(D, S, W, c, out=first, **kwargs)                          # prior_n = 0 into the scribbled buffers
    for k in KEYS:
        assert np.array_equal(bits(np_(again[k])), bits(plain[k])), k
    e.call_counter = t0
    again = e.search(D, S, W, c, out=first, prior_n=3, prior_v=5.0, **kwargs)   # and back to the longer table
    assert again is first and first["_logn"].numel() == n_log
    assert first["_workspace"].data_ptr() == ws and first["_policy_workspace"].data_ptr() == pws     # allocated once per out
    for k in KEYS:
        assert np.array_equal(bits(np_(again[k])), bits(keep[k])), k
    e.call_counter = t0
    e.search(D, S, W, c, out=first, diagnostics=True)                          # the uniform search shares `out`
    with pytest.raises(ValueError):
        e.search(D, S, 8, c, out=first, **kwargs)                              # another shape
