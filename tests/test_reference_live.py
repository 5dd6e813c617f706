"""Cross-check of the oracle against the UNMODIFIED reference on seeds of no other fixture, in configurations of no other
fixture: traces the reference produced on seeds, lanes and call counters drawn at random once, stored as
tests/golden/live_<id>.npz (tests/golden/generate_golden.py --live-only).  And, for the base configurations, one trace at the
edges of the Philox key and counter, tests/golden/edge_<env>.npz (--key-edges-only)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

CASES = [("rock", {}), ("rock", dict(board_size=11, num_rocks=11)), ("stochrock", {}), ("tag", {}),
         ("tag", dict(num_opponents=3)), ("tag", dict(move_prob=.3)), ("tag", dict(num_opponents=2, move_prob=.55)), ("battleship", {}), ("battleship", dict(board_size=(7, 9), max_len=4)),
         ("tiger", {}), ("network", {}), ("network", dict(n_machines=13, problem_type=3)),
         ("network", dict(n_machines=7, problem_type=2)),
         # the constructor parameters tests/test_gpu_env_params.py launches with
         ("stochrock", dict(p_move=.5)), ("stochrock", dict(p_move=.95)),
         ("tag", dict(move_prob=.5)), ("tag", dict(num_opponents=4, move_prob=.4)), ("tag", dict(obs_cells=64)),
         ("network", dict(n_machines=1, problem_type=2)), ("network", dict(n_machines=4, problem_type=3)),
         ("network", dict(n_machines=9, problem_type=1)), ("network", dict(n_machines=17, problem_type=1)),
         ("network", dict(n_machines=25, problem_type=3)), ("network", dict(n_machines=32, problem_type=2))]
IDS = ["%s-%d" % (c[0], i) for i, c in enumerate(CASES)]


def live_fixture(env, kw):
    """The stored traces of CASES' entry (env, kw), checked to be that configuration's."""
    g = np.load(os.path.join(GOLDEN, "live_%s.npz" % IDS[CASES.index((env, kw))]))
    assert str(g["env"]) == env
    assert json.loads(str(g["kwargs"])) == {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    return g


@pytest.mark.parametrize("env,kw", CASES, ids=IDS)
def test_fresh_seed_mode_a(oracle_lib, env, kw):
    """np.random.seed(s) trace of the reference == oracle on an emulated MT19937, on four stored seeds."""
    o = oracle_lib.OracleEnv(env, **kw)
    g = live_fixture(env, kw)
    runs = sorted({k.split("_")[0] for k in g.files if k.startswith("a")})
    assert len(runs) == 4
    for r in runs:
        seed, acts = int(g[r + "_seed"]), g[r + "_actions"]
        assert len(acts) == 400
        got = o.trace_mt(seed, acts)
        for k in ("ob", "reward", "done", "state_pre", "state", "reset_ob"):
            ref = g["%s_%s" % (r, k)]
            assert np.array_equal(ref, got[k].astype(ref.dtype)), (env, seed, k)


@pytest.mark.parametrize("env,kw", CASES, ids=IDS)
def test_fresh_seed_mode_b(oracle_lib, env, kw):
    """Philox-injected trace of the reference == oracle batch drivers, on two stored draws of seed / lanes / t."""
    o = oracle_lib.OracleEnv(env, **kw)
    g = live_fixture(env, kw)
    runs = sorted({k.split("_")[0] for k in g.files if k.startswith("b")})
    assert len(runs) == 2
    for r in runs:
        seed, lane0, t0, acts = int(g[r + "_seed"]), int(g[r + "_lane0"]), int(g[r + "_t0"]), g[r + "_actions"]
        L, T = acts.shape
        assert (L, T) == (12, 40)
        ref = {k: g["%s_%s" % (r, k)] for k in ("ob0", "ob", "reward", "done", "state")}
        st = o.new_state(L)
        assert np.array_equal(o.batch_reset(st, seed, lane0, t0), ref["ob0"])
        for i in range(T):
            ob, rew, done, _ = o.batch_step(st, acts[:, i], seed, lane0, t0 + 1 + i)
            assert np.array_equal(ob, ref["ob"][:, i]) and np.array_equal(done, ref["done"][:, i])
            assert np.array_equal(rew, ref["reward"][:, i].astype(o.reward_dtype))
            comp = np.array(ref["state"][:, i])
            if env == "tag":
                comp[:, -1] = np.maximum(comp[:, -1], -64)
            assert np.array_equal(o.batch_compact(st), comp), (env, i)


EDGE_CASES = [c for c in CASES if not c[1]]
EDGE_SEED, EDGE_LANE0, EDGE_T0 = 0x9E3779B97F4A7C15, (1 << 32) - 12, (1 << 32) - 7


@pytest.mark.parametrize("env,kw", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_key_and_counter_edges_mode_b(oracle_lib, env, kw):
    """Philox-injected trace of the reference == oracle batch drivers where every counter and key word is far from zero: both
    key words set (seed 0x9E3779B97F4A7C15), twelve lanes whose last is 0xFFFFFFFF (the quad-shared streams' counter word 0
    reaches 0x3FFFFFFF), reset at t = 2^32 - 7 so that the steps' call counter carries into its high word at step 7 of 40.
    tests/test_gpu_key_edges.py holds the kernels to the oracle at these coordinates."""
    o = oracle_lib.OracleEnv(env, **kw)
    g = np.load(os.path.join(GOLDEN, "edge_%s.npz" % env))
    assert str(g["env"]) == env and json.loads(str(g["kwargs"])) == kw
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as f:
        m = json.load(f)
    assert ["edge_%s" % env, env, kw] in m["key_edge_cases"]
    seed, lane0, t0, acts = int(g["seed"]), int(g["lane0"]), int(g["t0"]), g["actions"]
    assert (seed, lane0, t0) == (EDGE_SEED, EDGE_LANE0, EDGE_T0) == (m["key_edge"]["seed"], m["key_edge"]["lane0"], m["key_edge"]["t0"])
    L, T = acts.shape
    assert (L, T) == (12, 40) and lane0 + L == 1 << 32 and t0 < 1 << 32 < t0 + T
    ref = {k: g[k] for k in ("ob0", "ob", "reward", "done", "state")}
    st = o.new_state(L)
    assert np.array_equal(o.batch_reset(st, seed, lane0, t0), ref["ob0"])
    for i in range(T):
        ob, rew, done, bad = o.batch_step(st, acts[:, i], seed, lane0, t0 + 1 + i)
        assert bad == 0
        assert np.array_equal(ob, ref["ob"][:, i]) and np.array_equal(done, ref["done"][:, i]), (env, i)
        assert np.array_equal(rew, ref["reward"][:, i].astype(o.reward_dtype)), (env, i)
        comp = np.array(ref["state"][:, i])
        if env == "tag":
            comp[:, -1] = np.maximum(comp[:, -1], -64)
        assert np.array_equal(o.batch_compact(st), comp), (env, i)
