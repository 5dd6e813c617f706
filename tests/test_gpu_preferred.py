"""Rollouts under the env's preferred-action policy on the GPU (pomdp_rollout_preferred / pomdp_plan_preferred;
rollout / plan / plan_step(policy="preferred", history=...)) against the contract's CPU restatement
(tests/preferred_rollout_restatement.py), bit for bit.  Each case is one launch sequence.  test_preferred_host.py shows on the
oracle that the roots used here are not vacuous inputs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preferred_rollout_restatement as rr  # noqa: E402
from test_preferred_host import GPU_CASES, GPU_IDS, SEED, ROOTS, SIMS, DEPTH  # noqa: E402

pytestmark = pytest.mark.gpu

ENV_IDS = {"rock": "Rock-v0", "stochrock": "StochasticRock-v0", "tag": "Tag-v0", "battleship": "Battleship-v0", "tiger": "Tiger-v0",
           "network": "Network-v0"}
FIVE = ("ret", "n_steps", "first_action", "last_ob", "terminated")
# (roots, simulations per root, depth, particles per root (1: true states), lane_offset, call counter before planning or None)
SHAPES = [(ROOTS, SIMS, DEPTH, 1, 0, None),
          (ROOTS, SIMS, DEPTH, 256, 12, (1 << 32) + 5),
          (ROOTS, SIMS, DEPTH, 4, 0, None),
          (37, 150, 23, 1, 4, (1 << 33) - 2),                          # ragged: 5550 simulations, n % 4 == 2
          (37, 36, 23, 4, 8, None)]                                    # ragged particles: 1332 simulations
SHAPE_IDS = ["96x1024x64-true", "96x1024x64-P256-offset-t>2^32", "96x1024x64-P4", "ragged-true-offset-t>2^32", "ragged-P4-offset"]


def np_(t):
    return t.detach().cpu().numpy()


def u32(t):
    return np_(t).view(np.uint32)


def make(env, kw, n, **extra):
    import gym_pomdp_amd as gpa
    extra.setdefault("seed", SEED)
    extra.setdefault("auto_reset", False)
    if env in ("rock", "stochrock") and "use_heuristic" not in kw:
        extra.setdefault("use_heuristic", True)
    return gpa.make(ENV_IDS[env], batch_size=n, **kw, **extra)


def prepared(env, kw, R, prep, P=1, lane_offset=0, **extra):
    """an env of R lanes after reset() and `prep` real heuristic-policy steps, its History, and a particle belief that followed
    the same steps (P > 1)"""
    import gym_pomdp_amd as gpa
    e = make(env, kw, R, lane_offset=lane_offset, **extra)
    ob = e.reset()
    hist = gpa.History(e)
    b = None
    if P > 1:
        b = e.particle_belief(P)
        b.reset(ob)
    for _ in range(prep):
        a, ob, rew, done = e.heuristic_steps(hist, 1)
        if b is not None:
            b.update(a, ob)
    return e, hist, b


def roots_of(e, hist):
    """the roots' policy inputs as the restatement takes them (copies)"""
    belief = None if e.env_name != "rock" else {k: np_(v).copy() for k, v in e.belief.items()}
    history = dict(size=np_(hist._size).copy(), last_action=np_(hist.last_action).copy(), last_ob=np_(hist.last_ob).copy(),
                   total_sample=np_(hist.total_sample).copy(), total_move=np_(hist.total_move).copy())
    return belief, history, np_(hist.prev_ob).copy()


def raw_rollout(e, hist, states, R, P, sims, depth, lane0, t0):
    """pomdp_rollout_preferred itself, for the five per-simulation outputs from particles as well"""
    from gym_pomdp_amd import _native
    n = R * sims
    out = dict(ret=torch.empty(n, dtype=torch.float64, device=e.device), terminated=torch.empty(n, dtype=torch.uint8, device=e.device))
    for k in ("n_steps", "first_action", "last_ob"):
        out[k] = torch.empty(n, dtype=torch.int32, device=e.device)
    with torch.cuda.device(e.device):
        rc = e._lib.pomdp_rollout_preferred(_native.ENV_KIND[e.env_name], e._params_ref, states.data_ptr(), R, P, sims, depth,
                                            float(e._discount), *e._preferred_args(hist, n, out), e._seed, lane0, t0,
                                            *[out[k].data_ptr() for k in FIVE], e._stream())
    _native.check(rc, "pomdp_rollout_preferred")
    return out


@pytest.mark.parametrize("shape", range(len(SHAPES)), ids=SHAPE_IDS)
@pytest.mark.parametrize("case", range(len(GPU_CASES)), ids=GPU_IDS)
def test_rollout_and_plan_match_the_restatement(case, shape):
    from oracle import oracle_lib as ol
    env, kw, prep = GPU_CASES[case]
    R, sims, depth, P, lane_offset, counter = SHAPES[shape]
    o = ol.OracleEnv(env, **kw)
    e, hist, b = prepared(env, kw, R, prep, P, lane_offset)
    if counter is not None:
        e.call_counter = counter
    t0, lane0 = e.call_counter, lane_offset * sims
    belief, history, pob = roots_of(e, hist)
    state0 = u32(e.state).copy()
    states = state0 if b is None else u32(b.particles).copy()
    want_plan, want = rr.plan(o, states, belief, history, pob, R, P, sims, depth, e._discount, e._seed, lane0, t0, nthreads=ol.max_threads())
    got = raw_rollout(e, hist, e._state if b is None else b.particles, R, P, sims, depth, lane0, t0)
    for k in FIVE:
        assert np.array_equal(np_(got[k]), want[k]), (env, kw, SHAPE_IDS[shape], k)
    assert np_(got["ret"]).tobytes() == want["ret"].tobytes()
    p = e.plan(depth, sims, policy="preferred", history=hist, belief=b)
    assert e.call_counter == t0 + depth
    assert np_(p["sim_ret"]).tobytes() == want["ret"].tobytes() and np.array_equal(np_(p["sim_first_action"]), want["first_action"])
    assert np_(p["q"]).tobytes() == want_plan["q"].tobytes() and np_(p["value"]).tobytes() == want_plan["value"].tobytes()
    assert np.array_equal(np_(p["visits"]), want_plan["visits"]) and np.array_equal(np_(p["best"]), want_plan["best"])
    if P == 1:                                                          # rollout() from the live state: the same lanes when lane_offset * sims == lane0
        e.call_counter = t0
        r = e.rollout(depth, sims, lane_offset=lane0, policy="preferred", history=hist)
        for k in FIVE:
            assert np.array_equal(np_(r[k]).astype(want[k].dtype), want[k]), (k,)
    # nothing of the roots is written
    belief1, history1, pob1 = roots_of(e, hist)
    assert np.array_equal(u32(e.state), state0) and np.array_equal(pob1, pob)
    for k in history:
        assert np.array_equal(history1[k], history[k]), k
    if belief is not None:
        for k in belief:
            assert belief1[k].tobytes() == belief[k].tobytes(), k
    if b is not None:
        assert np.array_equal(u32(b.particles), states)


@pytest.mark.parametrize("env,kw", [("tiger", {}), ("network", {}), ("battleship", {}), ("rock", dict(use_heuristic=False))],
                         ids=["tiger", "network", "battleship", "rock-without-use_heuristic"])
def test_preferred_is_uniform_where_the_preferred_list_is_the_legal_list(env, kw):
    import gym_pomdp_amd as gpa
    R, sims, depth = 67, 100, 30
    e = make(env, kw, R, lane_offset=4)
    e.reset()
    hist = gpa.History(e)
    for _ in range(3):
        e.heuristic_steps(hist, 1) if env != "rock" else e.step(e.synthetic_actions())
    t0 = e.call_counter
    u = e.rollout(depth, sims)
    pu = e.plan(depth, sims)
    e.call_counter = t0
    r = e.rollout(depth, sims, policy="preferred", history=hist)
    pp = e.plan(depth, sims, policy="preferred", history=hist)
    for k in FIVE:
        assert np_(u[k]).tobytes() == np_(r[k]).tobytes(), (env, k)
    for k in ("q", "visits", "best", "value", "sim_ret", "sim_first_action"):
        assert np_(pu[k]).tobytes() == np_(pp[k]).tobytes(), (env, k)
    assert int(np_(u["n_steps"]).max()) > 1


@pytest.mark.parametrize("case", [0, 3], ids=["rock7x8", "tag"])
def test_sharding_invariance(case):
    env, kw, prep = GPU_CASES[case]
    R, sims, depth, cut = 48, 128, 32, 20
    e, hist, _ = prepared(env, kw, R, prep)
    whole = e.plan(depth, sims, policy="preferred", history=hist)
    parts = []
    for lo, hi in ((0, cut), (cut, R)):
        import gym_pomdp_amd as gpa
        s = make(env, kw, hi - lo, lane_offset=lo)
        s.reset()
        h = gpa.History(s)
        for _ in range(prep):
            s.heuristic_steps(h, 1)
        assert np.array_equal(u32(s.state), u32(e.state)[:, lo:hi])
        parts.append(s.plan(depth, sims, policy="preferred", history=h))
    for k in ("q", "visits", "best", "value"):
        assert np.concatenate([np_(p[k]) for p in parts]).tobytes() == np_(whole[k]).tobytes(), k


@pytest.mark.parametrize("case", [0, 3], ids=["rock7x8", "tag"])
def test_plan_step_keeps_history_statistics_and_belief_in_step(case):
    """plan_step(policy="preferred", belief=...) over several real steps against the same sequence made of the separate calls:
    plan, step (which updates the side statistics: pomdp_rock_belief_update), history.append, belief.update"""
    import gym_pomdp_amd as gpa
    env, kw, prep = GPU_CASES[case]
    R, sims, depth, P = 40, 64, 16, 16
    e1, h1, b1 = prepared(env, kw, R, prep, P)
    e2, h2, b2 = prepared(env, kw, R, prep, P)
    for step in range(4):
        ob1, rew1, done1, _, p1 = e1.plan_step(depth, sims, policy="preferred", history=h1, belief=b1)
        p2 = e2.plan(depth, sims, policy="preferred", history=h2, belief=b2)
        best = p2["best"].clone()
        ob2, rew2, done2, _ = e2.step(best)
        h2.append(gpa.Transition(h2.prev_ob, best, rew2, ob2, done2), auto_reset=False)
        h2.prev_ob.copy_(ob2)
        b2.update(best, ob2, rew2, done2)
        assert np.array_equal(np_(p1["best"]), np_(best)) and np_(p1["q"]).tobytes() == np_(p2["q"]).tobytes()
        assert np.array_equal(np_(ob1), np_(ob2)) and np.array_equal(np_(done1), np_(done2))
        assert np.array_equal(u32(e1.state), u32(e2.state)) and np.array_equal(u32(b1.particles), u32(b2.particles))
        a1, a2 = roots_of(e1, h1), roots_of(e2, h2)
        assert np.array_equal(a1[2], a2[2]) and np.array_equal(a1[2], np_(ob1))
        for k in a1[1]:
            assert np.array_equal(a1[1][k], a2[1][k]), k
        if a1[0] is not None:
            for k in a1[0]:
                assert a1[0][k].tobytes() == a2[0][k].tobytes(), k
    assert int(np_(h1._size).max()) == prep + 4


def test_refusals():
    import gym_pomdp_amd as gpa
    e = make("rock", {}, 8)
    other = make("rock", {}, 8)
    e.reset()
    other.reset()
    hist = gpa.History(e)
    with pytest.raises(ValueError):
        e.plan(4, 8, policy="preferred", history=gpa.History(e, max_size=5))
    with pytest.raises(ValueError):
        e.plan(4, 8, policy="preferred", history=hist, all_actions=True)
    with pytest.raises(ValueError):
        e.plan(4, 8, policy="preferred", history=hist, roots=e.state.clone())
    with pytest.raises(ValueError):
        e.rollout(4, 8, policy="preferred", history=gpa.History(other))
    with pytest.raises(ValueError):
        e.rollout(4, 8, policy="preferred")
    with pytest.raises(ValueError):
        e.plan(4, 8, policy="greedy", history=hist)
    with pytest.raises(ValueError):
        make("rock", {}, 8, auto_reset=True).plan_step(4, 8, policy="preferred", history=hist)
    t = e.call_counter
    e.plan(4, 8, policy="preferred", history=hist)                       # and the accepted form runs
    assert e.call_counter == t + 4
