"""Cross-check of the oracle against the UNMODIFIED reference on seeds of no other fixture, in configurations of no other
fixture: traces the reference produced on seeds, lanes and call counters drawn at random once, stored as
tests/golden/live_<id>.npz (tests/golden/generate_golden.py --live-only)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

CASES = [("rock", {}), ("rock", dict(board_size=11, num_rocks=11)), ("stochrock", {}), ("tag", {}),
         ("tag", dict(num_opponents=3)), ("tag", dict(move_prob=.3)), ("tag", dict(num_opponents=2, move_prob=.55)), ("battleship", {}), ("battleship", dict(board_size=(7, 9), max_len=4)),
         ("tiger", {}), ("network", {}), ("network", dict(n_machines=13, problem_type=3)),
         ("network", dict(n_machines=7, problem_type=2))]
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
