"""GPU parity: the HIP path (through the Python mirror, i.e. through the C ABI) against
(1) the committed golden traces of the reference and (2) the CPU oracle on seeded inputs.
Bit-exact for state words, observation, reward and done."""
import numpy as np
import pytest
import torch

from conftest import golden_cases, load_golden, saturate_tag_compact

pytestmark = pytest.mark.gpu

CASES = golden_cases()
ENV_IDS = {"rock": "Rock-v0", "stochrock": "StochasticRock-v0", "tag": "Tag-v0", "battleship": "Battleship-v0", "tiger": "Tiger-v0",
           "network": "Network-v0"}


def make_env(env, kw, **batch):
    import gym_pomdp_amd as gpa
    return gpa.make(ENV_IDS[env], **kw, **batch)


def np_(t):
    return t.detach().cpu().numpy()


def runs(lanes):
    L = len(lanes)
    starts = [0] + [i for i in range(1, L) if lanes[i] != lanes[i - 1] + 1] + [L]
    return list(zip(starts[:-1], starts[1:]))


def test_philox_kat_on_device():
    from gym_pomdp_amd import _native
    from oracle import philox_ref as px
    ck = torch.tensor([list(c) + list(k) for c, k, _ in px.KAT], dtype=torch.int64).to(torch.int32).cuda()
    # int64 -> int32 wraps the unsigned values
    out = torch.zeros((len(px.KAT), 4), dtype=torch.int32, device="cuda")
    _native.check(_native.lib().pomdp_philox_blocks(ck.data_ptr(), out.data_ptr(), len(px.KAT), None), "philox")
    torch.cuda.synchronize()
    got = np_(out).view(np.uint32)
    for row, (_, _, want) in zip(got, px.KAT):
        assert tuple(int(x) for x in row) == want


@pytest.mark.parametrize("case,env,kw", CASES, ids=[c[0] for c in CASES])
def test_golden_mode_b(case, env, kw):
    """HIP kernels == the unmodified reference driven by the same Philox words (fixture F3)."""
    g = load_golden("B", case)
    seed, t0 = int(g["seed"]), int(g["t0"])
    T = g["actions"].shape[1]
    for s, e in runs(g["lanes"]):
        n = e - s
        envb = make_env(env, kw, batch_size=n, seed=seed, lane_offset=int(g["lanes"][s]), auto_reset=True)
        envb.call_counter = t0
        ob0 = envb.reset()
        if n == 1:
            # an isolated lane runs through the scalar API (python scalars in and out, as the reference is used): the same
            # fixture rows, never a skip — a fixture regenerated with single-lane runs must not silently stop being checked
            assert ob0 == int(g["ob0"][s])
            assert np.array_equal(np_(envb.decode_state()), saturate_tag_compact(env, g["state0"][s:e]))
            for i in range(T):
                ob, rew, done, info = envb.step(int(g["actions"][s, i]))
                want_rew = float(np.float32(g["reward"][s, i])) if isinstance(rew, float) else int(g["reward"][s, i])
                assert (ob, rew, bool(done)) == (int(g["ob"][s, i]), want_rew, bool(g["done"][s, i])), (case, i)
                assert np.array_equal(np_(envb.decode_state()), saturate_tag_compact(env, g["state"][s:e, i])), (case, i)
            continue
        assert np.array_equal(np_(ob0), g["ob0"][s:e])
        assert np.array_equal(np_(envb.decode_state()), saturate_tag_compact(env, g["state0"][s:e]))
        for i in range(T):
            a = torch.as_tensor(g["actions"][s:e, i].astype(np.int32), device="cuda")
            ob, rew, done, info = envb.step(a)
            assert np.array_equal(np_(ob), g["ob"][s:e, i]), (case, i)
            assert np.array_equal(np_(rew), g["reward"][s:e, i].astype(np_(rew).dtype)), (case, i)
            assert np.array_equal(np_(done), g["done"][s:e, i].astype(bool)), (case, i)
            assert np.array_equal(np_(envb.decode_state()), saturate_tag_compact(env, g["state"][s:e, i])), (case, i)
        assert envb.invalid_action_count() == 0


ORACLE_CASES = [
    ("rock", {}, 65536, 64),                                        # BASELINE.json configs[1]
    ("rock", dict(board_size=15, num_rocks=15), 16384, 48),
    ("rock", dict(board_size=11, num_rocks=11), 8192, 32),
    ("tag", {}, 32768, 96),
    ("tag", dict(num_opponents=3), 8192, 64),
    ("battleship", dict(board_size=(10, 10), max_len=5), 8192, 160),
    ("battleship", {}, 16384, 64),
    ("tiger", {}, 32768, 32),
    ("network", {}, 32768, 32),
    ("network", dict(n_machines=31, problem_type=3), 4096, 16),
    ("stochrock", {}, 32768, 96),
    ("stochrock", dict(board_size=4, num_rocks=3), 4096, 64),
    ("stochrock", dict(board_size=15, num_rocks=15), 4096, 600),
    ("rock", {}, 4004, 40),                                         # ragged: not a multiple of the wave / workgroup size
    ("rock", dict(board_size=7, num_rocks=7), 1028, 40),            # odd K: last Philox block half used
    ("rock", dict(board_size=2, num_rocks=1), 260, 24),
    ("tag", dict(num_opponents=4), 516, 80),
    ("battleship", dict(board_size=(8, 6), max_len=4), 1020, 120),
]


@pytest.mark.parametrize("env,kw,n,T", ORACLE_CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(ORACLE_CASES)])
def test_hip_vs_oracle(oracle_lib, env, kw, n, T):
    """Same seeded inputs through the HIP path and the CPU oracle: identical words."""
    seed, lane0 = 20260929, 4096
    o = oracle_lib.OracleEnv(env, **kw)
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0)
    st = o.new_state(n)
    ob_o = o.batch_reset(st, seed, lane0, 0, nthreads=8)
    ob_g = e.reset()
    assert np.array_equal(np_(ob_g), ob_o)
    assert np.array_equal(np_(e.state).view(np.uint32), st)
    n_done = 0
    for t in range(1, T + 1):
        a = oracle_lib.synthetic_actions(n, seed ^ 0xABCDEF, lane0, t, o.n_actions, nthreads=8)
        a_g = e.synthetic_actions(seed=seed ^ 0xABCDEF)
        assert np.array_equal(np_(a_g), a)
        ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, nthreads=8)
        ob_g, rew_g, done_g, _ = e.step(a_g)
        assert np.array_equal(np_(ob_g), ob), t
        assert np.array_equal(np_(rew_g), rew), t
        assert np.array_equal(np_(done_g), done.astype(bool)), t
        assert np.array_equal(np_(e.state).view(np.uint32), st), t
        n_done += int(done.sum())
    if env not in ("network",):
        assert n_done > 0          # auto-reset path was exercised
    assert e.invalid_action_count() == 0


@pytest.mark.parametrize("env,kw", [("rock", {}), ("tag", {}), ("battleship", {}), ("tiger", {})])
def test_no_auto_reset_freezes(oracle_lib, env, kw):
    n, seed = 4096, 77
    o = oracle_lib.OracleEnv(env, **kw)
    e = make_env(env, kw, batch_size=n, seed=seed, auto_reset=False)
    st = o.new_state(n)
    o.batch_reset(st, seed, 0, 0)
    e.reset()
    done = np.zeros(n, np.uint8)
    for t in range(1, 60):
        a = oracle_lib.synthetic_actions(n, 5, 0, t, o.n_actions)
        ob, rew, done, _ = o.batch_step(st, a, seed, 0, t, auto_reset=False, done=done)
        ob_g, rew_g, done_g, _ = e.step(torch.as_tensor(a, device="cuda"))
        assert np.array_equal(np_(ob_g), ob) and np.array_equal(np_(rew_g), rew)
        assert np.array_equal(np_(done_g), done.astype(bool))
        assert np.array_equal(np_(e.state).view(np.uint32), st)
    assert done.sum() > 0


def test_network_sample_action_is_the_uniform_choice_over_the_legal_list(oracle_lib):
    """network.py:141-142: np.random.choice(_generate_legal()) with every action legal — the synthetic policy's draw at the
    env's call counter (a python int for one lane, as the reference returns)."""
    n, seed = 1000, 11
    e = make_env("network", {}, batch_size=n, seed=seed)
    e.reset()
    for t in (1, 2):
        a = e.sample_action()
        assert np.array_equal(np_(a), oracle_lib.synthetic_actions(n, seed, 0, t, 21))
        e.step(a)
    one = make_env("network", {}, batch_size=1, seed=seed)
    one.reset()
    assert one.sample_action() == int(oracle_lib.synthetic_actions(1, seed, 0, 1, 21)[0])


def test_odd_batch_sizes_without_synthetic_policy(oracle_lib):
    """batch sizes 1, 2, 3, 63, 65, 257 with host-provided actions (no multiple-of-4 requirement)."""
    for n in (1, 2, 3, 63, 65, 257):
        o = oracle_lib.OracleEnv("rock")
        e = make_env("rock", {}, batch_size=n, seed=8, lane_offset=3, auto_reset=True)
        st = o.new_state(n)
        ob0 = o.batch_reset(st, 8, 3, 0)
        r = e.reset()
        assert np.array_equal(np.atleast_1d(np_(r) if n > 1 else r), ob0)
        rs = np.random.RandomState(n)
        for t in range(1, 30):
            a = rs.randint(13, size=n).astype(np.int32)
            ob, rew, done, _ = o.batch_step(st, a, 8, 3, t)
            if n == 1:
                o1, r1, d1, _ = e.step(int(a[0]))
                assert (o1, r1, d1) == (int(ob[0]), int(rew[0]), bool(done[0]))
            else:
                og, rg, dg, _ = e.step(a)
                assert np.array_equal(np_(og), ob) and np.array_equal(np_(rg), rew) and np.array_equal(np_(dg), done.astype(bool))
            assert np.array_equal(np_(e.state).view(np.uint32), st)


def test_invalid_actions_are_counted_and_ignored():
    e = make_env("rock", {}, batch_size=8, seed=1)
    e.reset()
    before = np_(e.state).copy()
    a = torch.tensor([13, -1, 0, 99, 1, 2, 1 << 30, 5], dtype=torch.int32, device="cuda")
    ob, rew, done, _ = e.step(a)
    assert e.invalid_action_count() == 4
    bad = [0, 1, 3, 6]
    assert np.array_equal(np_(e.state)[:, bad], before[:, bad])
    assert np.all(np_(ob)[bad] == 0) and np.all(np_(rew)[bad] == 0) and not np_(done)[bad].any()


def test_sharding_invariance():
    """Two half-batches with lane offsets == one full batch (what makes multi-GPU exact)."""
    n, seed = 8192, 99
    full = make_env("rock", {}, batch_size=n, seed=seed)
    lo = make_env("rock", {}, batch_size=n // 2, seed=seed, lane_offset=0)
    hi = make_env("rock", {}, batch_size=n // 2, seed=seed, lane_offset=n // 2)
    for e in (full, lo, hi):
        e.reset()
    for t in range(20):
        a = full.synthetic_actions()
        r_full = full.step(a)
        r_lo = lo.step(a[: n // 2].contiguous())
        r_hi = hi.step(a[n // 2:].contiguous())
        for k in range(3):
            assert torch.equal(r_full[k], torch.cat([r_lo[k], r_hi[k]]))
        assert torch.equal(full.state, torch.cat([lo.state, hi.state], dim=1))


@pytest.mark.parametrize("action_seed", [None, 99], ids=["chained-policy", "separate-policy-key"])
def test_c_rollout_driver_equals_python_loop(action_seed):
    """pomdp_rollout_synthetic == a python loop over synthetic_actions() + step(), both when the policy
    shares the env's Philox key (actions for t+1 are produced inside the step launch) and when it does
    not (policy launch + step launch per step)."""
    n, seed = 16384, 5
    for env, kw in (("rock", {}), ("rock", dict(board_size=15, num_rocks=15)), ("rock", dict(board_size=4, num_rocks=3)),
                    ("stochrock", {}),
                    ("tag", {}), ("battleship", {}), ("tiger", {}), ("network", {})):
        a = make_env(env, kw, batch_size=n, seed=seed, reuse_buffers=True)
        b = make_env(env, kw, batch_size=n, seed=seed)
        a.reset()
        b.reset()
        scratch = torch.empty(n, dtype=torch.int32, device="cuda")
        a.rollout_synthetic(25, action_seed=action_seed, actions=scratch)
        # on return the buffer holds the policy's actions for the next call counter
        assert torch.equal(scratch, a.synthetic_actions(seed=action_seed))
        for _ in range(25):
            ob, rew, done, _ = b.step(b.synthetic_actions(seed=action_seed))
        assert a.call_counter == b.call_counter
        assert torch.equal(a.state, b.state), env
        assert torch.equal(a._ob, ob) and torch.equal(a._reward, rew) and torch.equal(a._done.view(torch.bool), done)


def test_scalar_env_mirrors_reference_errors():
    """batch_size=1: python scalars in/out, AssertionError / AttributeError like the reference
    (tests/golden/edge_cases.json)."""
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "edge_cases.json")) as f:
        edge = json.load(f)
    for env in ("rock", "tag", "battleship", "tiger", "network"):
        e = make_env(env, {})
        assert e.action_space.n == edge["%s.n_actions" % env]
        assert e.observation_space.n == edge["%s.n_obs" % env]
        with pytest.raises(AttributeError):
            e.step(0)
        assert edge["%s.step_before_reset" % env] == "AttributeError"
        ob = e.reset()
        assert isinstance(ob, int)
        for bad in (e.action_space.n, -1, 1.0):
            with pytest.raises(AssertionError):
                e.step(bad)
        ob, r, d, info = e.step(0)
        assert isinstance(ob, int) and isinstance(d, bool) and "state" in info
    e = make_env("rock", {}, seed=3)
    e.reset()
    ob, r, d, _ = e.step(3)          # WEST from x = 0: -100, done
    assert (ob, r, d) == (0, -100, True)
    with pytest.raises(AssertionError):
        e.step(0)
    assert edge["rock.step_after_done"] == "AssertionError"


def test_tiger_config1_rollout(oracle_lib):
    """BASELINE.json configs[0]: Tiger-v0 single env, 100-step random-action rollout."""
    e = make_env("tiger", {}, seed=11)
    o = oracle_lib.OracleEnv("tiger")
    st = o.new_state(1)
    assert e.reset() == int(o.batch_reset(st, 11, 0, 0)[0])
    t = 1
    rs = np.random.RandomState(0)
    for _ in range(100):
        a = int(rs.randint(3))
        ob, r, d, _ = e.step(a)
        ob_o, r_o, d_o, _ = o.batch_step(st, [a], 11, 0, t, auto_reset=False)
        assert (ob, r, d) == (int(ob_o[0]), int(r_o[0]), bool(d_o[0]))
        t += 1
        if d:
            assert e.reset() == int(o.batch_reset(st, 11, 0, t)[0])
            t += 1


def test_full_size_properties():
    """BASELINE.json metric size (2^20 lanes): properties that need no oracle run."""
    n, seed = 1 << 20, 123
    a_env = make_env("rock", {}, batch_size=n, seed=seed)
    b_env = make_env("rock", {}, batch_size=n, seed=seed)
    a_env.reset()
    b_env.reset()
    assert torch.equal(a_env.state, b_env.state)                      # determinism
    s = a_env.decode_state()
    assert torch.all(s[:, 0] == 0) and torch.all(s[:, 1] == 3)        # start cell
    frac_good = (s[:, 2:] == 1).double().mean().item()
    assert abs(frac_good - 0.5) < 2e-3                                # rocks are fair coins
    tot_done = 0
    for t in range(16):
        act = a_env.synthetic_actions()
        ob, rew, done, _ = a_env.step(act)
        ob2, rew2, done2, _ = b_env.step(act)
        assert torch.equal(ob, ob2) and torch.equal(rew, rew2) and torch.equal(done, done2)
        assert torch.equal(a_env.state, b_env.state)
        assert int(ob.min()) >= 0 and int(ob.max()) <= 2
        assert set(torch.unique(rew).tolist()) <= {-100, -10, 0, 10}
        assert torch.all(done == ((rew == -100) | ((rew == 10) & (act == 1))))   # rock.py:139-141, 193
        assert torch.all((ob == 0) | (act >= 5))                                  # only CHECK observes
        st = a_env.decode_state()
        assert int(st[:, :2].max()) <= 6 and int(st[:, 2:].min()) >= -1 and int(st[:, 2:].max()) <= 1
        tot_done += int(done.sum())
    assert 0.05 < tot_done / (16 * n) < 0.25                          # episodes last ~8 steps
    assert a_env.invalid_action_count() == 0
    # the same 2^20 lanes as 8 shards of 2^17 (what 8 GPUs would own): identical states, shard by shard
    from gym_pomdp_amd import sharding
    shards = []
    for r in range(8):
        off, cnt = sharding.shard_range(n, r, 8)
        e = make_env("rock", {}, batch_size=cnt, seed=seed, lane_offset=off)
        e.reset()
        for _ in range(16):
            e.step(e.synthetic_actions())
        shards.append(e.state)
    assert torch.equal(torch.cat(shards, dim=1), a_env.state)


# ---- planner hooks -------------------------------------------------------
def _rollout_cases():
    from conftest import golden_manifest
    return [(c[0], c[1], {k: (tuple(v) if isinstance(v, list) else v) for k, v in c[2].items()})
            for c in golden_manifest()["rollout_cases"]]


ROLLOUTS = _rollout_cases()


@pytest.mark.parametrize("case,env,kw", ROLLOUTS, ids=[c[0] for c in ROLLOUTS])
def test_rollouts_and_legal_lists_match_reference(case, env, kw):
    """HIP rollout / legal-action kernels == the reference's own _generate_legal() and step() loop
    (fixture rollout_*.npz), including the float64 discounted return."""
    import os
    from conftest import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "rollout_%s.npz" % case)))
    R, S = int(g["n_roots"]), int(g["sims_per_root"])
    e = make_env(env, kw, batch_size=R, seed=int(g["seed"]), lane_offset=int(g["root_lane0"]))
    e.call_counter = int(g["t_reset"])
    e.reset()
    assert np.array_equal(np_(e.decode_state()), saturate_tag_compact(env, g["root_state"]))
    lst, ln = e.legal_actions()
    A = e.action_space.n
    assert np.array_equal(np_(ln), g["root_legal_len"])
    assert np.array_equal(np_(lst), g["root_legal"][:, :A])
    assert np.all(g["root_legal"][:, A:] == -1)
    e.call_counter = int(g["t0"])
    before = e.state.clone()
    r = e.rollout(int(g["depth"]), sims_per_root=S, discount=float(g["discount"]),
                  all_actions=bool(g["all_actions"]), lane_offset=int(g["lane0"]))
    assert torch.equal(e.state, before)                                  # rollouts never touch the roots
    assert e.call_counter == int(g["t0"]) + int(g["depth"])
    assert np.array_equal(np_(r["ret"]), g["ret"])                       # IEEE double, bit-exact
    for k in ("n_steps", "first_action", "last_ob"):
        assert np.array_equal(np_(r[k]), g[k]), k
    assert np.array_equal(np_(r["terminated"]), g["terminated"].astype(bool))


def _plan_cases():
    from conftest import golden_manifest
    return [(c[0], c[1], {k: (tuple(v) if isinstance(v, list) else v) for k, v in c[2].items()})
            for c in golden_manifest()["plan_cases"]]


PLANS = _plan_cases()


@pytest.mark.parametrize("case,env,kw", PLANS, ids=[c[0] for c in PLANS])
def test_planning_step_matches_reference(case, env, kw):
    """BASELINE.json configs[4]'s planning step on the HIP path == fixture plan_*.npz: the reference's own step() under every
    simulation, the returns reduced in Python floats in the order include/pomdp_hip.h states (q / value bit for bit), then the
    reference's step() of the roots with the chosen actions."""
    import os
    from conftest import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "plan_%s.npz" % case)))
    R, S, depth = int(g["n_roots"]), int(g["sims_per_root"]), int(g["depth"])
    e = make_env(env, kw, batch_size=R, seed=int(g["seed"]), lane_offset=int(g["root_lane0"]), auto_reset=True)
    e.call_counter = int(g["t_reset"])
    e.reset()
    assert np.array_equal(np_(e.decode_state()), saturate_tag_compact(env, g["root_state"]))
    e.call_counter = int(g["t0"])
    before = e.state.clone()
    p = e.plan(depth, sims_per_root=S, discount=float(g["discount"]))
    assert torch.equal(e.state, before) and e.call_counter == int(g["t0"]) + depth
    assert np.array_equal(np_(p["sim_ret"]).view(np.uint64), g["sim_ret"].view(np.uint64))
    assert np.array_equal(np_(p["sim_first_action"]), g["sim_first_action"])
    assert np.array_equal(np_(p["visits"]), g["visits"]) and np.array_equal(np_(p["best"]), g["best"])
    assert np.array_equal(np_(p["q"]).view(np.uint64), g["q"].view(np.uint64))
    assert np.array_equal(np_(p["value"]).view(np.uint64), g["value"].view(np.uint64))
    # ... and the same through plan_step(): plan again from the same counter, then the real step
    e.call_counter = int(g["t0"])
    ob, rew, done, info, p2 = e.plan_step(depth, sims_per_root=S, discount=float(g["discount"]), out=p)
    assert p2 is p and np.array_equal(np_(p["best"]), g["best"])
    assert np.array_equal(np_(ob), g["ob"]) and np.array_equal(np_(done), g["done"].astype(bool))
    assert np.array_equal(np_(rew).astype(np.float64), g["reward"].astype(np_(rew).dtype).astype(np.float64))
    assert np.array_equal(np_(e.decode_state()), saturate_tag_compact(env, g["state"]))
    assert e.invalid_action_count() == 0 and e.call_counter == int(g["t0"]) + depth + 1


@pytest.mark.parametrize("env,kw,roots,sims,depth", [
    ("rock", dict(board_size=15, num_rocks=15), 96, 1024, 48),          # BASELINE.json configs[4] shape, scaled down
    ("rock", {}, 515, 200, 24),                                         # ragged: 200 = 3 chunks + 8, an odd number of roots
    ("rock", {}, 64, 2500, 16),                                         # more than two LDS tiles of 1024 simulations
    ("tag", {}, 300, 65, 30),
    ("battleship", dict(board_size=(10, 10), max_len=5), 37, 260, 40),  # 100 actions: two passes of 64 per chunk
    ("network", {}, 130, 96, 10),
    ("tiger", {}, 1000, 7, 8),
    ("tiger", {}, 9, 1, 3),
])
def test_plan_vs_oracle(oracle_lib, env, kw, roots, sims, depth):
    """plan() against the oracle's rollouts + or_plan_reduce on roots moved off their start states, float64 bit for bit;
    then a second planned step from the state the first one left (plan_step)."""
    seed, lane0 = 777, 4096
    o = oracle_lib.OracleEnv(env, **kw)
    e = make_env(env, kw, batch_size=roots, seed=seed, lane_offset=lane0, auto_reset=True)
    st = o.new_state(roots)
    o.batch_reset(st, seed, lane0, 0, nthreads=8)
    e.reset()
    for _ in range(2):
        a = oracle_lib.synthetic_actions(roots, 3, lane0, e.call_counter, o.n_actions)
        o.batch_step(st, a, seed, lane0, e.call_counter, nthreads=8)
        e.step(torch.as_tensor(a, device="cuda"))
    out = None
    for rep in range(2):
        t0 = e.call_counter
        r = o.batch_rollout(st, sims, depth, e._discount, seed, lane0 * sims, t0, nthreads=8)
        want = oracle_lib.plan_reduce(r["ret"], r["first_action"], roots, sims, o.n_actions)
        ob, rew, done, info, out = e.plan_step(depth, sims_per_root=sims, out=out)
        assert np.array_equal(np_(out["sim_ret"]).view(np.uint64), r["ret"].view(np.uint64))
        assert np.array_equal(np_(out["sim_first_action"]), r["first_action"])
        for k in ("q", "value"):
            assert np.array_equal(np_(out[k]).view(np.uint64), want[k].view(np.uint64)), (k, rep)
        for k in ("visits", "best"):
            assert np.array_equal(np_(out[k]), want[k]), (k, rep)
        ob_o, rew_o, done_o, bad = o.batch_step(st, want["best"], seed, lane0, t0 + depth, auto_reset=True, nthreads=8)
        assert np.array_equal(np_(ob), ob_o) and np.array_equal(np_(rew), rew_o) and np.array_equal(np_(done), done_o.astype(bool))
        assert np.array_equal(np_(e.state).view(np.uint32), st) and e.invalid_action_count() == bad
    assert (np_(out["visits"]).sum(axis=1) == sims).all()


def test_plan_does_not_depend_on_the_sharding_and_handles_no_simulation():
    """Root r is global lane lane_offset + r and its simulations global lanes (lane_offset + r) * S ..: two shards of a root
    set reproduce the unsharded plan exactly (whole roots never straddle a shard).  depth = 0: no simulation takes a step —
    best = -1, value = 0, nothing visited."""
    kw = dict(board_size=11, num_rocks=11)
    S, depth = 132, 12
    whole = make_env("rock", kw, batch_size=24, seed=9, lane_offset=40)
    whole.reset()
    p = whole.plan(depth, sims_per_root=S)
    for lo, hi in ((0, 8), (8, 24)):
        part = make_env("rock", kw, batch_size=hi - lo, seed=9, lane_offset=40 + lo)
        part.reset()
        assert torch.equal(part.state, whole.state[:, lo:hi])
        q = part.plan(depth, sims_per_root=S)
        for k in ("q", "visits", "best", "value"):
            assert torch.equal(q[k], p[k][lo:hi]), k
        assert torch.equal(q["sim_ret"], p["sim_ret"][lo * S:hi * S])
    z = whole.plan(0, sims_per_root=S)
    assert (np_(z["best"]) == -1).all() and (np_(z["value"]) == 0).all() and (np_(z["visits"]) == 0).all() and (np_(z["q"]) == 0).all()
    assert (np_(z["sim_first_action"]) == -1).all()
    with pytest.raises(ValueError):
        make_env("rock", {}, batch_size=4, seed=1, lane_offset=3).plan(4, sims_per_root=5)    # first simulation lane 15: not on a quad


def test_plan_through_the_c_abi(oracle_lib):
    """pomdp_plan / pomdp_plan_reduce called directly: the reduction over caller-supplied simulation results (a wider stride,
    columns past the action count left alone, value = NULL), and the argument checks."""
    import ctypes as C
    from gym_pomdp_amd import _native
    L = _native.lib()
    R, S, A, stride = 5, 300, 13, 16
    rng = np.random.RandomState(3)
    ret = rng.randn(R * S)
    fa = rng.randint(-1, A, R * S).astype(np.int32)
    d_ret, d_fa = torch.as_tensor(ret, device="cuda"), torch.as_tensor(fa, device="cuda")
    q = torch.full((R, stride), 7.5, dtype=torch.float64, device="cuda")
    visits = torch.full((R, stride), -3, dtype=torch.int32, device="cuda")
    best = torch.zeros(R, dtype=torch.int32, device="cuda")
    po = _native.PlanOut(q=q.data_ptr(), visits=visits.data_ptr(), best=best.data_ptr(), value=None, stride=stride, reserved=0)
    assert L.pomdp_plan_reduce(d_ret.data_ptr(), d_fa.data_ptr(), R, S, A, C.byref(po), None) == 0
    torch.cuda.synchronize()
    want = oracle_lib.plan_reduce(ret, fa, R, S, A)
    assert np.array_equal(np_(q)[:, :A].view(np.uint64), want["q"].view(np.uint64)) and (np_(q)[:, A:] == 7.5).all()
    assert np.array_equal(np_(visits)[:, :A], want["visits"]) and (np_(visits)[:, A:] == -3).all()
    assert np.array_equal(np_(best), want["best"])
    assert L.pomdp_plan_reduce(d_ret.data_ptr(), d_fa.data_ptr(), R, S, 256, C.byref(po), None) == -1     # actions beyond a byte
    assert L.pomdp_plan_reduce(d_ret.data_ptr(), d_fa.data_ptr(), R, S, 20, C.byref(po), None) == -1      # stride < n_actions
    assert L.pomdp_plan_reduce(None, d_fa.data_ptr(), R, S, A, C.byref(po), None) == -1
    assert L.pomdp_plan_reduce(d_ret.data_ptr(), d_fa.data_ptr(), R, 0, A, C.byref(po), None) == -1
    assert L.pomdp_plan_reduce(d_ret.data_ptr(), d_fa.data_ptr(), 0, S, A, C.byref(po), None) == 0
    e = make_env("rock", {}, batch_size=R, seed=1)
    e.reset()
    bad = _native.PlanOut(q=q.data_ptr(), visits=visits.data_ptr(), best=None, value=None, stride=stride, reserved=0)
    args = (_native.ENV_KIND["rock"], e._params_ref, e.state.data_ptr(), R, S, 8, .95, 0, 1, 0, 0, d_ret.data_ptr(), d_fa.data_ptr())
    assert L.pomdp_plan(*args, C.byref(bad), None) == -1
    assert L.pomdp_plan(*args, None, None) == -1
    assert L.pomdp_plan(*args, C.byref(po), None) == 0
    torch.cuda.synchronize()
    assert (np_(visits)[:, :A].sum(axis=1) == S).all()
    # pomdp_rollout's optional outputs (ABI 14): NULL n_steps / last_ob / terminated
    assert L.pomdp_rollout(_native.ENV_KIND["rock"], e._params_ref, e.state.data_ptr(), R, S, 8, .95, 0, 1, 0, 0, d_ret.data_ptr(), None,
                           d_fa.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("env,kw,roots,sims,depth", [
    ("rock", dict(board_size=15, num_rocks=15), 64, 1024, 48),          # BASELINE.json configs[4] shape, scaled down
    ("rock", {}, 4096, 8, 32),
    ("tag", {}, 2048, 16, 40),
    ("battleship", dict(board_size=(10, 10), max_len=5), 256, 16, 110),
    ("network", {}, 1024, 16, 12),
    ("tiger", {}, 4096, 4, 10),
])
def test_rollout_vs_oracle(oracle_lib, env, kw, roots, sims, depth):
    seed, lane0 = 4242, 1 << 16
    o = oracle_lib.OracleEnv(env, **kw)
    e = make_env(env, kw, batch_size=roots, seed=seed, lane_offset=lane0)
    st = o.new_state(roots)
    o.batch_reset(st, seed, lane0, 0, nthreads=8)
    e.reset()
    for _ in range(3):                                                  # move the roots off the start state
        a = oracle_lib.synthetic_actions(roots, 1, lane0, e.call_counter, o.n_actions)
        o.batch_step(st, a, seed, lane0, e.call_counter, nthreads=8)
        e.step(torch.as_tensor(a, device="cuda"))
    assert np.array_equal(np_(e.state).view(np.uint32), st)
    lists, lens = o.batch_legal(st)
    lst, ln = e.legal_actions()
    assert np.array_equal(np_(ln), lens) and np.array_equal(np_(lst), lists[:, : e.action_space.n])
    t0 = e.call_counter
    want = o.batch_rollout(st, sims, depth, e._discount, seed, lane0, t0, nthreads=8)
    got = e.rollout(depth, sims_per_root=sims)
    assert np.array_equal(np_(got["ret"]), want["ret"])
    for k in ("n_steps", "first_action", "last_ob"):
        assert np.array_equal(np_(got[k]), want[k]), k
    assert np.array_equal(np_(got["terminated"]), want["terminated"].astype(bool))


def test_reference_state_encodings():
    """_encode_state mirrors the reference's array encodings (rock.py:196-212, 376-381; tag.py:158-165)."""
    e = make_env("rock", {}, batch_size=64, seed=1)
    e.reset()
    for _ in range(5):
        e.step(e.synthetic_actions())
    d = e.decode_state()
    enc = e._encode_state()
    assert enc.shape == (64, 9)
    assert torch.equal(enc[:, 0], d[:, 1] * 7 + d[:, 0]) and torch.equal(enc[:, 1:], d[:, 2:])
    t = make_env("tag", dict(num_opponents=2), batch_size=32, seed=1)
    t.reset()
    enc = t._encode_state()
    assert enc.shape == (32, 3) and enc.dtype == torch.int32 and int(enc.min()) >= 0 and int(enc.max()) <= 28


def test_network_ansi_render(capsys):
    e = make_env("network", {}, seed=2)
    e.reset()
    e.render()
    assert capsys.readouterr().out.strip() == "N: 10, S: 0\tNull"
    e.step(5)
    e.render()
    out = capsys.readouterr().out.strip()
    assert out.startswith("N: ") and out.endswith("M: 2 A: 1")


@pytest.mark.parametrize("env", ["rock", "tag", "battleship", "tiger", "network"])
def test_scalar_loop_equals_the_batched_path_and_sync_entry_points(env, oracle_lib):
    """batch_size=1 (pomdp_step_sync / pomdp_reset_sync: outputs in pinned host memory, published through a polled flag) over
    a few hundred steps with resets in between against the oracle, step for step; and pomdp_reset_sync on a batch (n != 1:
    launch + hipStreamSynchronize) against reset()."""
    from gym_pomdp_amd import _native
    seed = 41
    e = make_env(env, {}, seed=seed)
    o = oracle_lib.OracleEnv(env)
    st = o.new_state(1)
    rs = np.random.RandomState(3)
    t = 0
    assert e.reset() == int(o.batch_reset(st, seed, 0, t)[0])
    for _ in range(300):
        t += 1
        a = int(rs.randint(o.n_actions))
        ob, rew, done, bad = o.batch_step(st, np.array([a], np.int32), seed, 0, t, auto_reset=False, done=np.zeros(1, np.uint8))
        ob_g, rew_g, done_g, _ = e.step(a)
        assert (ob_g, float(rew_g), bool(done_g)) == (int(ob[0]), float(rew[0]), bool(done[0])), (env, t)
        if done_g:
            t += 1
            assert e.reset() == int(o.batch_reset(st, seed, 0, t)[0]), (env, t)
    n = 4096
    b = make_env(env, {}, batch_size=n, seed=seed, reuse_buffers=True)
    ob_ref = b.reset().clone()
    st_ref = b.state.clone()
    b.state.zero_()
    ob2 = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    rc = _native.lib().pomdp_reset_sync(_native.ENV_KIND[env], b._params_ref, b._state.data_ptr(), ob2.data_ptr(), n, seed, 0, 0, None)
    _native.check(rc, "pomdp_reset_sync")
    assert torch.equal(ob2, ob_ref) and torch.equal(b.state, st_ref)
    assert _native.lib().pomdp_reset_sync(99, b._params_ref, b._state.data_ptr(), ob2.data_ptr(), n, seed, 0, 0, None) == -1


def test_scalar_planner_hooks():
    e = make_env("rock", {}, seed=5)
    e.reset()
    assert e._generate_legal() == [1, 0, 2, 5, 6, 7, 8, 9, 10, 11, 12]   # start (0,3): no WEST, no rock underfoot
    s0 = e._get_init_state()
    assert s0.shape == (1, 1)
    e._set_state(s0)
    assert torch.equal(e.state, s0)


def _prob_cases():
    from conftest import golden_manifest
    return [(c[0], c[1], {k: (tuple(v) if isinstance(v, list) else v) for k, v in c[2].items()})
            for c in golden_manifest()["prob_cases"]]


PROBS = _prob_cases()


@pytest.mark.parametrize("case,env,kw", PROBS, ids=[c[0] for c in PROBS])
def test_compute_prob_matches_reference(case, env, kw):
    """pomdp_compute_prob == the reference's _compute_prob for every observation value (fixture prob_*.npz)."""
    import os
    from conftest import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "prob_%s.npz" % case)))
    seed, t0, lane0 = int(g["seed"]), int(g["t0"]), int(g["lanes"][0])
    L, T, n_obs = g["prob"].shape
    frozen = make_env(env, kw, batch_size=L, seed=seed, lane_offset=lane0, auto_reset=False)   # keeps terminal states
    live = make_env(env, kw, batch_size=L, seed=seed, lane_offset=lane0, auto_reset=True)
    for e in (frozen, live):
        e.call_counter = t0
        e.reset()
    for i in range(T):
        a = torch.as_tensor(g["actions"][:, i].astype(np.int32), device="cuda")
        frozen.set_state(live.state)                 # same pre-step state, no lane frozen
        frozen.call_counter = live.call_counter
        ob, _, _, _ = frozen.step(a)
        assert np.array_equal(np_(ob), g["ob"][:, i])
        assert np.array_equal(np_(frozen.decode_state()), saturate_tag_compact(env, g["state_pre"][:, i]))
        for q in range(n_obs):
            got = frozen.compute_prob(a, torch.full((L,), q, dtype=torch.int32, device="cuda"))
            assert np.array_equal(np_(got), g["prob"][:, i, q]), (case, i, q)
        live.step(a)
    s = make_env("tiger", {}, seed=1)
    s.reset()
    s.step(2)
    assert s._compute_prob(2, None, 2) == 0.0 and s._compute_prob(0, None, 2) == 1.0


def test_randomised_configs_vs_oracle(oracle_lib):
    """Property test: random (env config, batch size, seed, lane offset, call counter, auto-reset mode) — the HIP
    path and the oracle stay word-for-word identical.  Seeded, so a failure is reproducible."""
    rs = np.random.RandomState(20260929)
    configs = [("rock", dict(board_size=b, num_rocks=k)) for b, k in ((2, 1), (4, 3), (7, 7), (7, 8), (11, 11), (15, 15))]
    configs += [("stochrock", dict(board_size=b, num_rocks=k)) for b, k in ((4, 3), (7, 8), (15, 15))]
    configs += [("tag", dict(num_opponents=k)) for k in (1, 2, 3, 4)]
    configs += [("battleship", dict(board_size=bs, max_len=m)) for bs, m in (((5, 5), 3), ((6, 4), 2), ((8, 8), 4),
                                                                             ((10, 10), 5), ((11, 11), 6), ((16, 7), 5))]
    configs += [("tiger", {})]
    configs += [("network", dict(n_machines=m, problem_type=p)) for m, p in ((4, 3), (10, 3), (16, 3), (5, 1), (32, 2),
                                                                            (31, 3))]
    for trial in range(36):
        env, kw = configs[trial % len(configs)]
        n = int(rs.choice([1, 5, 64, 100, 255, 256, 257, 1000, 4096])) * 4
        seed = int(rs.randint(0, 2 ** 62))
        lane0 = int(rs.randint(0, 2 ** 28)) * 4
        t0 = int(rs.randint(0, 2 ** 36))
        auto = bool(rs.randint(2))
        o = oracle_lib.OracleEnv(env, **kw)
        e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, auto_reset=auto)
        e.call_counter = t0
        st = o.new_state(n)
        assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, t0)), (env, kw)
        done = np.zeros(n, np.uint8)
        for t in range(t0 + 1, t0 + 1 + 24):
            a = oracle_lib.synthetic_actions(n, seed + 1, lane0, t, o.n_actions)
            ob, rew, done, _ = o.batch_step(st, a, seed, lane0, t, auto_reset=auto, done=done)
            ob_g, rew_g, done_g, _ = e.step(torch.as_tensor(a, device="cuda"))
            ctx = (env, kw, n, seed, lane0, t, auto)
            assert np.array_equal(np_(ob_g), ob), ctx
            assert np.array_equal(np_(rew_g), rew), ctx
            assert np.array_equal(np_(done_g), done.astype(bool)), ctx
            assert np.array_equal(np_(e.state).view(np.uint32), st), ctx


def test_episode_statistics_match_the_reference_probes():
    """Size-independent check at scale: under uniform random actions the done rate per step is 1 / (mean episode
    length).  SURVEY.md §8d records the reference's mean episode lengths as probed by running it: RockSample(7,8)
    ~8.3 steps, Tag ~430.  BattleShip 10x10 (14 ship cells, revisits allowed) is a coupon collector over 14 of 100
    cells: 100 * H_14 = 325.2 steps — the reference itself gives 327.9 +- 7.5 over 300 episodes (SURVEY's "~285" was
    a rougher probe)."""
    def done_rate(env, kw, n, burn, steps):
        e = make_env(env, kw, batch_size=n, seed=2024, reuse_buffers=True)
        e.reset()
        e.rollout_synthetic(burn)
        tot = torch.zeros((), dtype=torch.int64, device="cuda")
        for _ in range(steps):
            e.rollout_synthetic(1)
            tot += e._done.sum()
        return tot.item() / (n * steps)

    r = done_rate("rock", {}, 1 << 18, 64, 64)
    assert abs(1 / r - 8.3) < 0.4, 1 / r
    r = done_rate("tag", {}, 1 << 18, 2000, 200)
    assert abs(1 / r - 430) < 45, 1 / r
    r = done_rate("battleship", dict(board_size=(10, 10), max_len=5), 1 << 16, 1500, 400)
    assert abs(1 / r - 100 * sum(1.0 / k for k in range(1, 15))) < 12, 1 / r


@pytest.mark.parametrize("env,kw,log2n,policy_seed", [
    ("rock", {}, 32, None),                                    # the ABI's maximum: 2^32 - 1024 lanes, 73 GB of columns
    ("rock", {}, 27, None),                                    # 2.4 GB of columns in one batch
    ("rock", dict(board_size=7, num_rocks=7), 19, None),       # two-lanes-per-thread path, odd K
    ("rock", dict(board_size=15, num_rocks=15), 19, None),     # two-lanes-per-thread launch, per-sub-batch fallback
    ("stochrock", {}, 20, None),
    ("rock", {}, 20, 777),                                     # distinct policy key: plain two-lanes-per-thread launches
    ("tag", {}, 20, None),                                     # Tag's pooled pass (flights + resets + chained policy)
    ("tag", {}, 19, 777),                                      # the same from plain launches
    ("tag", dict(num_opponents=2), 19, None),                  # two lanes per thread, general multi-opponent path
])
def test_large_batch_windows_vs_oracle(oracle_lib, env, kw, log2n, policy_seed):
    """Big batches (the launch geometry switches to two lanes per thread at 2^19 lanes): windows of lanes at the
    start, in the middle and at the very end are checked word for word against the oracle."""
    n, seed, steps, win = (1 << log2n) - (1024 if log2n == 32 else 0), 31337, (4 if log2n == 32 else 8), 2048
    e = make_env(env, kw, batch_size=n, seed=seed, reuse_buffers=True)
    e.reset()
    e.rollout_synthetic(steps, action_seed=policy_seed)
    torch.cuda.synchronize()
    o = oracle_lib.OracleEnv(env, **kw)
    aseed = seed if policy_seed is None else policy_seed
    for lane0 in (0, (n >> 1) - 1024, n - win):
        st = o.new_state(win)
        o.batch_reset(st, seed, lane0, 0, nthreads=4)
        for t in range(1, steps + 1):
            a = oracle_lib.synthetic_actions(win, aseed, lane0, t, o.n_actions, nthreads=4)
            ob, rew, done, _ = o.batch_step(st, a, seed, lane0, t, nthreads=4)
        sl = slice(lane0, lane0 + win)
        assert np.array_equal(np_(e.state[:, sl]).view(np.uint32), st), lane0
        assert np.array_equal(np_(e._ob[sl]), ob) and np.array_equal(np_(e._reward[sl]), rew)
        assert np.array_equal(np_(e._done[sl]), done)
    del e
    torch.cuda.empty_cache()


@pytest.mark.parametrize("env,kw", [("rock", {}), ("tag", {}), ("rock", dict(board_size=15, num_rocks=15))],
                         ids=["rock_7_8", "tag_1", "rock_15_15"])
def test_ragged_batch_on_the_pooled_path(oracle_lib, env, kw):
    """A batch that ends inside a workgroup (2^18 + 260 lanes, lane ids past 2^31): the out-of-range threads of the last
    two-lanes-per-thread workgroup take part in the pooled passes but must not leak into any result."""
    n, seed, lane0, steps, win = (1 << 18) + 260, 4242, (1 << 31) + 4, 12, 1024
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
    guard = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")      # right behind nothing we own: just a canary
    e.reset()
    e.rollout_synthetic(steps)
    torch.cuda.synchronize()
    o = oracle_lib.OracleEnv(env, **kw)
    off = n - win
    st = o.new_state(win)
    o.batch_reset(st, seed, lane0 + off, 0, nthreads=4)
    for t in range(1, steps + 1):
        a = oracle_lib.synthetic_actions(win, seed, lane0 + off, t, o.n_actions, nthreads=4)
        ob, rew, done, _ = o.batch_step(st, a, seed, lane0 + off, t, nthreads=4)
    assert np.array_equal(np_(e.state[:, off:]).view(np.uint32), st)
    assert np.array_equal(np_(e._ob[off:]), ob) and np.array_equal(np_(e._reward[off:]), rew)
    assert np.array_equal(np_(e._done[off:]), done)
    assert bool((guard == 0x5A5A5A5A).all()) and e.invalid_action_count() == 0


def test_tag_pooled_resets_including_the_rejection_fallback(oracle_lib):
    """Every lane of a 2^18-lane Tag batch tags its opponent in the same step, so all of them start a new episode
    inside the pooled pass: the resets read the 5-bit fields of the lanes' words of the pooled quad blocks (ABI 13; the lanes
    whose masked-rejection draws run past the six fields are pinned by test_tag_quad_word_rare_paths).  All against the oracle."""
    n, seed, lane0 = 1 << 18, 99, 1 << 19
    e = make_env("tag", {}, batch_size=n, seed=seed, lane_offset=lane0)
    e.reset()
    cell = (torch.arange(n, device="cuda", dtype=torch.int64) * 7) % 29
    packed = (cell | (cell << 5) | (1 << 25)).to(torch.int32).reshape(1, n)
    e.set_state(packed)
    t = e.call_counter
    ob, rew, done, _ = e.step(torch.full((n,), 4, dtype=torch.int32, device="cuda"))
    o = oracle_lib.OracleEnv("tag")
    st = np_(packed).view(np.uint32).copy()
    ob_o, rew_o, done_o, _ = o.batch_step(st, np.full(n, 4, np.int32), seed, lane0, t, nthreads=4)
    assert bool(done.all()) and done_o.all()
    assert np.array_equal(np_(ob), ob_o) and np.array_equal(np_(rew), rew_o)
    assert np.array_equal(np_(e.state).view(np.uint32), st)
    # rejections were exercised: some lanes' quad word has a field above 28 among the first two
    from oracle import philox_ref as px
    lanes = np.arange(lane0, lane0 + 4096)
    rej = np.array([any(((int(px.tag_step_words(seed, int(l), t)[0]) >> (5 * k)) & 31) > 28 for k in range(2)) for l in lanes])
    assert rej.sum() > 0


def test_tag_quad_word_rare_paths():
    """Fixture ties_tag.npz (the reference's own results, tests/golden/find_ties.py --tag) on the device: auto-resets whose
    draws run past the quad word's six fields, flights decided by the double's low word — through the one-lane-per-thread
    step kernel (n = 4) and the pooled two-lanes-per-thread one (2^18 lanes)."""
    import os
    from conftest import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "ties_tag.npz")))
    seed = int(g["seed"])
    for i, lane in enumerate(g["lanes"]):
        lane = int(lane)
        for n in (4, 1 << 18):
            base = lane & ~3 if n == 4 else max(0, (lane & ~3) - (n // 2))
            col = lane - base
            e = make_env("tag", {}, batch_size=n, seed=seed, lane_offset=base)
            e.reset()
            assert np.array_equal(np_(e.decode_state()[col]), g["state0"][i]), (lane, n)
            ob, rew, done, _ = e.step(torch.full((n,), 4, dtype=torch.int32, device="cuda"))
            assert (int(ob[col]), float(rew[col]), int(done[col])) == (int(g["ob"][i]), float(g["reward"][i]), int(g["done"][i])), (lane, n)
            assert np.array_equal(np_(e.decode_state()[col]), g["state"][i]), (lane, n)


def test_tag_quad_word_rare_paths_in_the_fused_loops():
    """The same fixture through the FUSED consumers of Tag's word contract, which a tape of the caller's actions can now steer
    onto the tie lanes: tag_steps_quad_kernel with and without its step table (2^19 lanes; 16 steps / 1 step per launch) and
    the general one-lane-per-thread loop (8 lanes: step_w / fresh_w on the time-shared quad block).  Row 0 — TAG everywhere, as
    in the fixture — against the reference's outcome; every row and the final state against a python loop over step()."""
    import os
    from conftest import GOLDEN
    from gym_pomdp_amd import _native
    g = dict(np.load(os.path.join(GOLDEN, "ties_tag.npz")))
    seed = int(g["seed"])
    for i, lane in enumerate(g["lanes"]):
        lane = int(lane)
        for n, k, kernel in ((8, 1, "steps_kernel<"), (8, 16, "steps_kernel<"), (1 << 19, 1, "tag_steps_quad_kernel<false"), (1 << 19, 16, "tag_steps_quad_kernel<true")):
            base = lane & ~7 if n == 8 else max(0, (lane & ~1023) - (n // 2))
            col = lane - base
            e = make_env("tag", {}, batch_size=n, seed=seed, lane_offset=base)
            ref = make_env("tag", {}, batch_size=n, seed=seed, lane_offset=base)
            e.reset(), ref.reset()
            tape = torch.randint(0, 5, (k, n), dtype=torch.uint8, device="cuda")
            tape[0] = 4
            cols = e.decode_trajectory(e.collect_tape(tape, layout="packed"), k)
            assert _native.lib().pomdp_last_fused_kernel().decode().startswith(kernel), (n, k)
            assert (int(cols["ob"][0, col]), float(cols["reward"][0, col]), int(cols["done"][0, col])) == \
                (int(g["ob"][i]), float(g["reward"][i]), int(g["done"][i])), (lane, n, k)
            for s in range(k):
                ob, rew, done, _ = ref.step(tape[s].to(torch.int32))
                assert torch.equal(cols["ob"][s], ob) and torch.equal(cols["reward"][s], rew) and torch.equal(cols["done"][s], done), (lane, n, k, s)
                if s == 0:
                    assert np.array_equal(np_(ref.decode_state()[col]), g["state"][i]), (lane, n)
            assert torch.equal(e.state, ref.state), (lane, n, k)


def test_network_state_words_with_stray_bits_step_alike_in_every_launch_shape():
    """A Network state word is n_machines bits; set_state() refuses anything above them, but a C caller could hand such a
    word in.  Every launch shape — the one-lane step kernel, the quad step kernel (2^19 lanes), the fused loops — reads the
    machines only: the same draws, observation and reward as for the clean word."""
    for n in (1000, 1 << 19):
        clean = make_env("network", {}, batch_size=n, seed=11, reuse_buffers=True)
        dirty = make_env("network", {}, batch_size=n, seed=11, reuse_buffers=True)
        clean.reset(), dirty.reset()
        a = clean.synthetic_actions().clone()
        clean.step(a), dirty.step(a)                                  # some machines down
        dirty._state.bitwise_or_(torch.tensor(0x7FF << 12, dtype=torch.int32, device="cuda"))     # bits 12 .. 22: no machine of the ten
        for t in range(3):
            a = clean.synthetic_actions().clone()
            want, got = clean.step(a), dirty.step(a)
            assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]), (n, t)
            assert torch.equal(clean.state & 0x3FF, dirty.state & 0x3FF), (n, t)
        dirty._state.bitwise_or_(torch.tensor(0x7FF << 12, dtype=torch.int32, device="cuda"))
        tw, tg = clean.collect_synthetic(20, layout="packed"), dirty.collect_synthetic(20, layout="packed")
        assert torch.equal(tw["traj"], tg["traj"]) and torch.equal(clean.state & 0x3FF, dirty.state & 0x3FF), n


def test_split_layout_ties():
    """The 2^-27 path of RockSample's split word layout: lanes (found by tests/golden/find_ties.py) where a reset or
    sensor draw is undecided by its high word, so the kernel has to generate the low-word block.  Expected values
    come from the reference itself (fixture ties_rock.npz)."""
    import os
    from conftest import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "ties_rock.npz")))
    seed = int(g["seed"])
    for i, lane in enumerate(g["lanes"]):
        lane = int(lane)
        for n in (4, 1 << 18):                      # one-lane-per-thread path and the pooled two-lanes-per-thread path
            base = lane & ~3 if n == 4 else max(0, (lane & ~3) - (n // 2))
            col = lane - base
            e = make_env("rock", {}, batch_size=n, seed=seed, lane_offset=base)
            e.reset()
            assert np.array_equal(np_(e.decode_state()[col]), g["state0"][i]), (lane, n)
            a = torch.zeros(n, dtype=torch.int32, device="cuda")
            a[col] = int(g["actions"][i])
            ob, rew, done, _ = e.step(a)
            assert (int(ob[col]), int(rew[col]), int(done[col])) == (int(g["ob"][i]), int(g["reward"][i]), int(g["done"][i])), (lane, n)


def test_auto_reset_ties():
    """A done step's auto-reset starts the new episode from the step's own sensor block; fixture ties_rock_auto.npz holds
    lanes (found by tests/golden/find_ties.py --auto) where a rock of that new episode is decided by the LOW word, with the
    reference's outcome.  Through the one-lane-per-thread step kernel, the pooled two-lanes-per-thread one and the
    quad-per-thread one (2^19 lanes)."""
    import os
    from conftest import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "ties_rock_auto.npz")))
    seed = int(g["seed"])
    for i, lane in enumerate(g["lanes"]):
        lane = int(lane)
        for n in (4, 1 << 18, 1 << 19):
            base = lane & ~3 if n == 4 else max(0, (lane & ~3) - (n // 2))
            col = lane - base
            e = make_env("rock", {}, batch_size=n, seed=seed, lane_offset=base)
            e.reset()
            assert np.array_equal(np_(e.decode_state()[col]), g["state0"][i]), (lane, n)
            a = torch.full((n,), 5, dtype=torch.int32, device="cuda")            # everybody else CHECKs rock 0
            a[col] = int(g["actions"][i])
            ob, rew, done, _ = e.step(a)
            assert (int(ob[col]), int(rew[col]), int(done[col])) == (int(g["ob"][i]), int(g["reward"][i]), 1), (lane, n)
            assert np.array_equal(np_(e.decode_state()[col]), g["state"][i]), (lane, n)


def test_network_split_layout_ties():
    """The 2^-27 path of Network's split word layout (fixture ties_network.npz: the reference on lanes where a failure
    or observation draw is undecided by its high word)."""
    import os
    from conftest import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "ties_network.npz")))
    seed = int(g["seed"])
    for i, lane in enumerate(g["lanes"]):
        lane = int(lane)
        base = lane & ~3
        e = make_env("network", {}, batch_size=4, seed=seed, lane_offset=base)
        e.reset()
        ob, rew, done, _ = e.step(torch.zeros(4, dtype=torch.int32, device="cuda"))
        col = lane - base
        assert int(ob[col]) == int(g["ob"][i]) and float(rew[col]) == float(np.float32(g["reward"][i])), lane
        assert np.array_equal(np_(e.decode_state()[col]), g["state"][i]), lane


# ---- heuristic policy support -----------------------------------------------------------
from conftest import OracleHeuristicOps, golden_manifest, heuristic_replay  # noqa: E402
from history_window_restatement import window_sums  # noqa: E402

HEUR = [tuple(c) for c in golden_manifest().get("heuristic_cases", [])]


class HipHeuristicOps(object):
    """The ops heuristic_replay drives, on the HIP path through the Python mirror (History, preferred_actions,
    select_target, pick_actions, step with tracked side statistics)."""

    def __init__(self, env, kw):
        self.env_name, self.kw = env, kw
        self.is_rock = env in ("rock", "stochrock")

    def reset(self, n, seed, lane0, t):
        from gym_pomdp_amd import History
        extra = dict(use_heuristic=True) if self.is_rock else {}
        self.e = make_env(self.env_name, dict(self.kw, **extra), batch_size=n, seed=seed, lane_offset=lane0, auto_reset=True)
        self.e.call_counter = t
        ob = self.e.reset()
        self.h = History(self.e, max_size=getattr(self, "max_size", None))
        return np_(ob)

    def preferred(self):
        l, n = self.e._generate_preferred(self.h)
        return np_(l), np_(n)

    def legal(self):
        l, n = self.e.legal_actions()
        return np_(l), np_(n)

    def target(self):
        return np_(self.e.select_target())

    def pick(self, lists, lens, t):
        assert self.e.call_counter == t
        l = torch.as_tensor(np.ascontiguousarray(lists, np.int32), device="cuda")
        n = torch.as_tensor(np.ascontiguousarray(lens, np.int32), device="cuda")
        return np_(self.e.pick_actions(l, n))

    def step(self, a, t):
        assert self.e.call_counter == t
        self._a = torch.as_tensor(a, device="cuda")
        ob, rew, done, _ = self.e.step(self._a)
        self._ob, self._done = ob, done
        return np_(ob), np_(rew), np_(done).astype(np.uint8)

    def reset_ob(self):
        d = np_(self.e.decode_state())
        return np.where((d[:, 1:-1] == d[:, :1]).any(axis=1), 29, d[:, 0]).astype(np.int32)

    def track(self, prev_ob, a, ob, done):
        from gym_pomdp_amd import Transition
        self.h.append(Transition(torch.as_tensor(prev_ob, device="cuda"), self._a, None, self._ob, self._done))

    def compact(self):
        return np_(self.e.decode_state())

    def belief(self):
        return {k: np_(v) for k, v in self.e.belief.items()}


@pytest.mark.parametrize("case,env,kw", HEUR, ids=[c[0] for c in HEUR])
def test_heuristic_golden(case, env, kw):
    """Side statistics (float64, bit for bit), _generate_preferred, _select_target and the picked actions of the HIP
    path == the reference run with use_heuristic=True on injected Philox words."""
    from oracle import oracle_lib as ol
    heuristic_replay(case, env, ol.OracleEnv(env, **kw), HipHeuristicOps(env, kw))


@pytest.mark.parametrize("env,kw,n,T,max_size", [("rock", {}, 16384, 96, None), ("rock", dict(board_size=15, num_rocks=15), 8192, 96, None),
                                                 ("stochrock", {}, 4096, 128, None), ("tag", {}, 8192, 128, None),
                                                 ("rock", {}, 8192, 96, 8), ("rock", dict(board_size=11, num_rocks=11), 4096, 96, 0),
                                                 ("rock", dict(board_size=15, num_rocks=15), 4096, 128, 30), ("tag", {}, 4096, 64, 2),
                                                 ("rock", {}, 2048, 160, 100), ("tag", {}, 1024, 96, 300)],
                         ids=["rock_7_8", "rock_15_15", "stochrock_7_8", "tag_1", "rock_7_8-hist8", "rock_11_11-hist0",
                              "rock_15_15-hist30", "tag_1-hist2", "rock_7_8-hist100", "tag_1-hist300"])
def test_heuristic_vs_oracle_at_scale(env, kw, n, T, max_size):
    """A device-resident heuristic-policy loop (preferred -> pick -> step -> statistics -> history) against the oracle's
    restatement, every lane following its own preferred list; with max_size the planner's history is History(max_size)
    (rock.py:533-544), which the oracle keeps as the reference does — a list of records with pop(0)."""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv(env, **kw)
    seed, lane0 = 0xFEED5EED, (1 << 20) - 512
    cpu, gpu = OracleHeuristicOps(ol, o), HipHeuristicOps(env, kw)
    cpu.max_size = gpu.max_size = max_size
    prev_c, prev_g = cpu.reset(n, seed, lane0, 0), gpu.reset(n, seed, lane0, 0)
    assert np.array_equal(prev_c, prev_g)
    is_rock = env in ("rock", "stochrock")
    n_done = 0
    for t in range(1, T + 1):
        (lc, nc), (lg, ng) = cpu.preferred(), gpu.preferred()
        assert np.array_equal(nc, ng), t
        assert np.array_equal(lc[:, : lg.shape[1]], lg), t
        if is_rock:
            assert np.array_equal(cpu.target(), gpu.target()), t
        ac, ag = cpu.pick(lc, nc, t), gpu.pick(lg, ng, t)
        assert np.array_equal(ac, ag), t
        oc, og = cpu.step(ac, t), gpu.step(ag, t)
        for x, y in zip(oc, og):
            assert np.array_equal(x, y.astype(x.dtype)), t
        cpu.track(prev_c, ac, oc[0], oc[2])
        gpu.track(prev_g, ag, og[0], og[2])
        prev_c = prev_g = np.where(oc[2] != 0, 0 if is_rock else cpu.reset_ob(), oc[0]).astype(np.int32)
        n_done += int(oc[2].sum())
        assert np.array_equal(cpu.compact(), saturate_tag_compact(env, gpu.compact())), t
        if is_rock:
            bc, bg = cpu.belief(), gpu.belief()
            for k in bc:
                same = (bc[k] == bg[k]) | ((bc[k] != bc[k]) & (bg[k] != bg[k]))
                assert same.all(), (t, k)
        # (a bounded history's sums: the oracle walks its records when asked — window_sums is that walk, as arrays)
        ws = dict(zip(("total_sample", "total_move"), window_sums(cpu.h, o.n_actions - 5))) if is_rock and max_size is not None else {}
        for k in ("size", "last_action", "last_ob") + (("total_sample", "total_move") if max_size is None or is_rock else ()):
            assert np.array_equal(ws.get(k, getattr(cpu.h, k)), np_(getattr(gpu.h, "_size" if k == "size" else k))), (t, k)
        if max_size is not None:
            assert int(cpu.h.size.max()) <= max_size + 1
        if is_rock:      # the derived words the policy reads == the per-rock tests on the oracle's full arrays
            K = o.n_actions - 5
            w = (1 << np.arange(K, dtype=np.int64))[:, None]
            ok = (bc["measured"] < 5) & (np.abs(bc["count"]) < 2) & (bc["prob_valuable"] > 0) & (bc["prob_valuable"] < 1)
            assert np.array_equal((ok * w).sum(axis=0), np_(gpu.e._tracker.check_ok).astype(np.int64) & 0xFFFFFFFF), t
            mo = np_(gpu.h.move_ok).astype(np.int64) & 0xFFFFFFFF        # bit j: total_move[j] >= 0, bit 16 + j: total_sample[j] > 0
            tm, ts = ws.get("total_move", cpu.h.total_move), ws.get("total_sample", cpu.h.total_sample)
            assert np.array_equal(((tm >= 0) * w).sum(axis=0), mo & 0xFFFF), t
            assert np.array_equal(((ts > 0) * w).sum(axis=0), mo >> 16), t
    # (a policy that forgets its old CHECKs keeps re-measuring: with a short window no episode need end inside T steps)
    assert n_done > 0 or max_size is not None


def test_set_belief_refreshes_the_derived_word():
    """set_belief() (the statistics part of the reference's _set_state, rock.py:200-203) recomputes check_ok."""
    e = make_env("rock", dict(use_heuristic=True), batch_size=256, seed=3)
    e.reset()
    g = torch.Generator(device="cpu").manual_seed(5)
    K, n = 8, 256
    b = dict(count=torch.randint(-3, 4, (K, n), generator=g, dtype=torch.int32),
             measured=torch.randint(0, 8, (K, n), generator=g, dtype=torch.int32),
             lkv=torch.rand((K, n), generator=g, dtype=torch.float64), lkw=torch.rand((K, n), generator=g, dtype=torch.float64),
             prob_valuable=torch.rand((K, n), generator=g, dtype=torch.float64).round(decimals=1))
    e.set_belief(b)
    ok = (b["measured"] < 5) & (b["count"].abs() < 2) & (b["prob_valuable"] > 0) & (b["prob_valuable"] < 1)
    want = (ok.to(torch.int64) << torch.arange(K)[:, None]).sum(dim=0)
    assert torch.equal(e._tracker.check_ok.cpu().to(torch.int64), want)
    for k in b:
        assert torch.equal(e.belief[k].cpu(), b[k])


@pytest.mark.parametrize("env,kw,n,T,auto", [("rock", {}, 8192, 64, True), ("rock", dict(board_size=15, num_rocks=15), 4096, 64, True),
                                             ("stochrock", {}, 4096, 96, True), ("tag", {}, 8192, 96, True),
                                             ("tag", dict(num_opponents=2), 4096, 96, False), ("rock", {}, 4096, 48, False),
                                             ("tiger", {}, 4096, 24, True), ("battleship", {}, 4096, 40, True),
                                             ("network", {}, 4096, 16, True),
                                             ("rock", dict(hist=8), 8192, 96, True), ("rock", dict(hist=0), 4096, 48, False),
                                             ("tag", dict(hist=1), 4096, 48, True)],
                         ids=["rock_7_8", "rock_15_15", "stochrock_7_8", "tag_1", "tag_2_noreset", "rock_7_8_noreset", "tiger",
                              "battleship_5_5", "network_10", "rock_7_8-hist8", "rock_7_8-hist0-noreset", "tag_1-hist1"])
def test_fused_heuristic_steps_match_the_call_sequence(env, kw, n, T, auto):
    """pomdp_heuristic_steps (one launch per step) == preferred_actions -> pick_actions -> step (+ side statistics) ->
    History.append issued separately, on every output, the state, the statistics and the history sums — also with a
    bounded History(max_size) (`hist`), whose window the two paths keep in step."""
    from gym_pomdp_amd import History, Transition
    kw = dict(kw)
    max_size = kw.pop("hist", None)
    is_rock = env in ("rock", "stochrock")
    extra = dict(use_heuristic=True) if is_rock else {}
    mk = lambda: make_env(env, dict(kw, **extra), batch_size=n, seed=77, lane_offset=4096, auto_reset=auto)  # noqa: E731
    ea, eb = mk(), mk()
    oa, ob_ = ea.reset(), eb.reset()
    ha, hb = History(ea, max_size=max_size), History(eb, max_size=max_size)
    prev = oa.clone()
    for t in range(T):
        lst, ln = ea.preferred_actions(ha) if (is_rock or env == "tag") else ea.legal_actions()
        a = ea.pick_actions(lst, ln)
        if not auto:                              # frozen lanes: the fused path reports action -1 and leaves them alone
            frozen = ea._done.bool().clone()
        o, r, d, _ = ea.step(a)
        ha.append(Transition(prev, a, r, o, d))
        if env == "tag":
            dec = ea.decode_state()
            reset_ob = torch.where((dec[:, 1:-1] == dec[:, :1]).any(dim=1), torch.full_like(dec[:, 0], 29), dec[:, 0]).to(torch.int32)
        else:
            reset_ob = torch.full_like(o, 2 if env == "tiger" else 0)
        prev = torch.where(d & auto, reset_ob, o)
        fa, fo, fr, fd = eb.heuristic_steps(hb, 1)
        if auto:
            assert torch.equal(fa, a), t
        else:
            assert torch.equal(fa[~frozen], a[~frozen]) and bool((fa[frozen] == -1).all()), t
        assert torch.equal(fo, o) and torch.equal(fr, r) and torch.equal(fd, d), t
        assert torch.equal(ea.state, eb.state), t
        if not auto:
            live = ~frozen
            assert torch.equal(hb._size[live], ha._size[live]), t
            continue
        assert torch.equal(hb.prev_ob, prev), t
        for k in ("_size", "last_action", "last_ob", "total_sample", "total_move", "head", "ring"):
            assert torch.equal(getattr(ha, k), getattr(hb, k)), (t, k)
        if max_size is not None:
            assert int(ha._size.max()) <= max_size + 1
        if is_rock:
            for k in ea.belief:
                x, y = ea.belief[k], eb.belief[k]
                assert bool(((x == y) | (x.isnan() & y.isnan() if x.is_floating_point() else False)).all()), (t, k)
    assert int(ea._done.sum()) >= 0


def test_encoded_state_round_trips(capsys):
    """Host-side views: _encode_state -> _decode_state -> set_state reproduces the packed state
    (RockSample one and two words, Tag with several opponents); the text renderers print."""
    for env, kw in (("rock", {}), ("rock", dict(board_size=15, num_rocks=15)), ("tag", dict(num_opponents=3))):
        e = make_env(env, kw, batch_size=4096, seed=5)
        e.reset()
        for _ in range(6):
            e.step(e.synthetic_actions())
        packed = e.state.clone()
        enc = e._encode_state()
        dec = e._decode_state(enc)
        if env == "tag":    # the reference's decoding is lossy: num_opp becomes the number of listed opponents (tag.py:171-173)
            assert torch.equal(dec & 0x01FFFFFF, packed & 0x01FFFFFF) and bool(((dec >> 25) == 3).all())
        else:
            assert torch.equal(dec, packed), (env, kw)
        e.set_state(dec)
        assert torch.equal(e.state, dec)
    t = make_env("tiger", {}, batch_size=1, seed=1)
    t.reset()
    t.step(2)
    t.render()
    n = make_env("network", {}, batch_size=1, seed=1)
    n.reset()
    n.step(3)
    n.render()
    out = capsys.readouterr().out
    assert "tiger is in state" in out and "M: 1 A: 1" in out


@pytest.mark.parametrize("env,kw,auto", [("rock", {}, True), ("rock", {}, False), ("tag", {}, True), ("stochrock", {}, True)],
                         ids=["rock_auto", "rock_frozen", "tag_auto", "stochrock_auto"])
def test_heuristic_returns_accumulate_like_the_reference_loop(env, kw, auto):
    """`r += rw * discount; discount *= env._discount` of the reference's rollout loop (rock.py:569-570), per lane on the
    device == the same float64 recurrence applied on the host to the per-step rewards, bit for bit; ret_done carries the
    return of each finished episode."""
    from gym_pomdp_amd import History, Returns
    is_rock = env in ("rock", "stochrock")
    n, T = 4096, 80
    e = make_env(env, dict(kw, **(dict(use_heuristic=True) if is_rock else {})), batch_size=n, seed=11, auto_reset=auto)
    e.reset()
    h, R = History(e), Returns(e)
    ret, disc = np.zeros(n), np.ones(n)
    ret_done = np.full(n, np.nan)
    frozen = np.zeros(n, bool)
    for t in range(T):
        _, _, rew, done = e.heuristic_steps(h, 1, returns=R)
        r, d = np_(rew).astype(np.float64), np_(done)
        live = ~frozen
        term = disc * r
        acc = ret + term
        ret_done = np.where(live & d, acc, ret_done)
        fresh = live & d & auto
        ret = np.where(live, np.where(fresh, 0.0, acc), ret)
        disc = np.where(live, np.where(fresh, 1.0, disc * e._discount), disc)
        if not auto:
            frozen |= d
        assert np.array_equal(np_(R.ret), ret) and np.array_equal(np_(R.disc), disc), t
        both_nan = np.isnan(np_(R.ret_done)) & np.isnan(ret_done)
        assert ((np_(R.ret_done) == ret_done) | both_nan).all(), t
    assert np.isfinite(ret_done).sum() > 0 or env == "stochrock"


FUSE_CASES = [("rock", {}, 1 << 20, True), ("rock", dict(board_size=7, num_rocks=7), (1 << 20) + 1024, True),   # four lanes per thread,
              ("rock", dict(board_size=11, num_rocks=11), 1 << 20, True), ("rock", dict(board_size=4, num_rocks=3), 1 << 20, True),  # table-driven step
              ("rock", dict(board_size=15, num_rocks=15), 1 << 20, True),                                            # ... with two state words
              ("rock", {}, (1 << 18) + 260, True), ("rock", {}, 4100, True), ("rock", {}, (1 << 18) + 4, False),
              ("rock", dict(board_size=15, num_rocks=15), 1 << 18, True), ("stochrock", {}, 1 << 18, True),
              ("tag", {}, (1 << 18) + 516, True), ("tag", {}, 5000, False), ("tag", dict(num_opponents=3), 1 << 18, True),
              ("tag", {}, 1 << 20, True), ("tag", dict(num_opponents=2), 1 << 20, True),                              # a quad per thread / not
              ("battleship", {}, 20000, True), ("battleship", dict(board_size=(10, 10), max_len=5), 8192, True),
              ("tiger", {}, 30000, True), ("tiger", {}, 30000, False), ("network", {}, 30000, True),
              ("tiger", {}, 1 << 20, True), ("network", {}, 1 << 20, True)]                                          # a quad per thread / not


@pytest.mark.parametrize("env,kw,n,auto", FUSE_CASES, ids=["%s-%d-%s" % (c[0], c[2], "auto" if c[3] else "frozen") for c in FUSE_CASES])
def test_fused_steps_leave_what_per_step_launches_leave(env, kw, n, auto):
    """pomdp_rollout_synthetic with POMDP_FUSE_STEPS (up to 64 steps per launch, state and action in registers between
    steps) == the same steps launched one by one: state, action scratch, ob, reward, done and the error counter, after
    runs that cross the 64-step launch boundary, for both launch geometries and with frozen (no auto-reset) lanes."""
    steps = [1, 3, 64, 65, 7]
    a = make_env(env, kw, batch_size=n, seed=2718, lane_offset=8, auto_reset=auto, reuse_buffers=True)
    b = make_env(env, kw, batch_size=n, seed=2718, lane_offset=8, auto_reset=auto, reuse_buffers=True)
    a.reset()
    b.reset()
    for k in steps:
        a.rollout_synthetic(k, fuse=False)
        b.rollout_synthetic(k, fuse=True)
        for name in ("_state", "_action_scratch", "_ob", "_reward", "_done"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (env, kw, n, auto, k, name)
    assert a.invalid_action_count() == b.invalid_action_count() == 0
    assert a.call_counter == b.call_counter


HEUR_FUSE_CASES = [("rock", dict(hist=90), 2048, True),              # a window longer than a launch (any max_size since round 4)
                   ("rock", {}, 4096 + 1, True), ("rock", dict(board_size=15, num_rocks=15), 2048 + 2, True), ("tag", {}, 4096 + 3, True),   # n % 4 != 0:
                   ("stochrock", {}, 1024 + 3, False),                               # the padding threads of the last quad supply blocks
                   ("rock", {}, 8192 + 12, True), ("rock", {}, 4096, False), ("rock", dict(board_size=15, num_rocks=15), 4096, True),
                   ("stochrock", {}, 4096, True), ("tag", {}, 8192, True), ("tag", dict(num_opponents=2), 4096, False),
                   ("battleship", {}, 4096, True), ("tiger", {}, 4096, True), ("network", {}, 4096, True),
                   ("rock", dict(hist=5), 4096 + 12, True), ("rock", dict(board_size=15, num_rocks=15, hist=40), 4096, True)]


@pytest.mark.parametrize("env,kw,n,auto", HEUR_FUSE_CASES,
                         ids=["%s%s-%d-%s" % (c[0], "-hist%d" % c[1]["hist"] if "hist" in c[1] else "", c[2], "auto" if c[3] else "frozen") for c in HEUR_FUSE_CASES])
def test_heuristic_steps_in_one_launch_equal_single_step_launches(env, kw, n, auto):
    """env.heuristic_steps(history, k) runs up to 64 steps per launch with the lane's history words, derived words and
    running return in registers: every array it owns must end up exactly as after k one-step launches."""
    from gym_pomdp_amd import History, Returns
    kw = dict(kw)
    max_size = kw.pop("hist", None)                     # History(max_size): the window travels through the multi-step launch too
    is_rock = env in ("rock", "stochrock")
    mk = lambda: make_env(env, dict(kw, **(dict(use_heuristic=True) if is_rock else {})), batch_size=n, seed=31, lane_offset=64,  # noqa: E731
                          auto_reset=auto)
    ea, eb = mk(), mk()
    ea.reset()
    eb.reset()
    ha, hb, ra, rb = History(ea, max_size=max_size), History(eb, max_size=max_size), Returns(ea), Returns(eb)
    for k in (1, 3, 64, 65, 7):
        for _ in range(k):
            outs_a = ea.heuristic_steps(ha, 1, returns=ra)
        outs_b = eb.heuristic_steps(hb, k, returns=rb)
        ctx = (env, kw, n, auto, k)
        for x, y in zip(outs_a, outs_b):
            assert torch.equal(x, y), ctx
        assert torch.equal(ea.state, eb.state), ctx
        for name in ("_size", "last_action", "last_ob", "total_sample", "total_move", "move_ok", "prev_ob", "head", "ring"):
            assert torch.equal(getattr(ha, name), getattr(hb, name)), ctx + (name,)
        for name in ("ret", "disc", "ret_done"):
            x, y = getattr(ra, name), getattr(rb, name)
            assert bool(((x == y) | (x.isnan() & y.isnan())).all()), ctx + (name,)
        if is_rock:
            assert torch.equal(ea._tracker.check_ok, eb._tracker.check_ok), ctx
            for name in ea.belief:
                x, y = ea.belief[name], eb.belief[name]
                assert bool(((x == y) | (x.isnan() & y.isnan() if x.is_floating_point() else False)).all()), ctx + (name,)
    assert ea.call_counter == eb.call_counter


COLLECT_CASES = [("rock", {}, 1 << 20, 66), ("rock", dict(board_size=15, num_rocks=15), 1 << 20, 40), ("rock", {}, (1 << 16) + 260, 70), ("rock", {}, 4100, 130),
                 ("rock", dict(board_size=15, num_rocks=15), 1 << 16, 70), ("stochrock", {}, 1 << 14, 70),
                 ("tag", {}, (1 << 16) + 516, 70), ("tag", {}, 1 << 20, 70), ("tag", dict(num_opponents=3), 1 << 14, 70), ("battleship", {}, 20000, 70),
                 ("tiger", {}, 30000, 70), ("network", {}, 30000, 70)]


@pytest.mark.parametrize("env,kw,n,steps", COLLECT_CASES, ids=["%s-%d" % (c[0], c[2]) for c in COLLECT_CASES])
def test_collected_trajectories_equal_the_per_step_calls(env, kw, n, steps):
    """env.collect_synthetic(k) keeps every step's results: row s of action / ob / reward / done must be what
    synthetic_actions() + step() return at that call (itself checked against the oracle above), across the 64-step
    launch boundary and for every launch geometry; the state and the call counter end where the loop ends."""
    a = make_env(env, kw, batch_size=n, seed=99, lane_offset=12, reuse_buffers=True)
    b = make_env(env, kw, batch_size=n, seed=99, lane_offset=12, reuse_buffers=True)
    a.reset()
    b.reset()
    a.rollout_synthetic(3, fuse=True)                      # start from a call counter other than the reset's
    b.rollout_synthetic(3, fuse=True)
    tr = b.collect_synthetic(steps)
    check = sorted(set(range(0, steps, 9)) | {0, 1, 62, 63, 64, 65, steps - 1})
    for s in range(steps):
        act = a.synthetic_actions()
        ob, rew, done, _ = a.step(act)
        if s in check:
            ctx = (env, kw, n, s)
            assert torch.equal(tr["action"][s], act), ctx
            assert torch.equal(tr["ob"][s], ob), ctx
            assert torch.equal(tr["reward"][s], rew), ctx
            assert torch.equal(tr["done"][s], done), ctx
    assert torch.equal(tr["action"][steps], a.synthetic_actions())
    assert torch.equal(a.state, b.state)
    assert a.call_counter == b.call_counter
    assert b.invalid_action_count() == 0
    again = b.collect_synthetic(steps, out=tr)             # buffers are reusable
    assert again is tr


def test_collect_needs_auto_reset_and_a_reset():
    e = make_env("tiger", {}, batch_size=64, seed=1, auto_reset=False)
    with pytest.raises(AttributeError):
        e.collect_synthetic(4)
    e.reset()
    with pytest.raises(ValueError):
        e.collect_synthetic(4)


@pytest.mark.parametrize("env,n,pitch,steps", [("rock", 5000, 5120, 67), ("rock", 1 << 20, (1 << 20) + 64, 20),
                                               ("tag", 1 << 20, (1 << 20) + 8, 20), ("tiger", 1 << 20, (1 << 20) + 4, 20),
                                               ("rock", 1 << 20, (1 << 20) + 2, 18)],      # a pitch the 16-byte stores cannot take
                         ids=["rock-5000", "rock-quad", "tag-quad", "tiger-quad", "rock-odd-pitch"])
def test_collect_row_pitch_through_the_c_abi(env, n, pitch, steps):
    """pomdp_collect_synthetic with pitch > n: rows start every `pitch` elements and the padding is left alone (also in the
    launches where a thread owns four consecutive lanes and stores 16 bytes at a time)."""
    from gym_pomdp_amd import _native
    a = make_env(env, {}, batch_size=n, seed=5, reuse_buffers=True)
    b = make_env(env, {}, batch_size=n, seed=5, reuse_buffers=True)
    a.reset()
    b.reset()
    act = torch.full((steps + 1, pitch), -7, dtype=torch.int32, device="cuda")
    ob = torch.full((steps, pitch), -7, dtype=torch.int32, device="cuda")
    rew = torch.full((steps, pitch), -7, dtype=b._reward.dtype, device="cuda")
    done = torch.full((steps, pitch), 9, dtype=torch.uint8, device="cuda")
    rc = _native.lib().pomdp_collect_synthetic(
        _native.ENV_KIND[b.env_name], b._params_ref, b._state.data_ptr(), act.data_ptr(), ob.data_ptr(), rew.data_ptr(),
        done.data_ptr(), b._err.data_ptr(), n, b._seed, b.lane_offset, b._t, steps, pitch, _native.POMDP_AUTO_RESET, None)
    _native.check(rc, "pomdp_collect_synthetic")
    torch.cuda.synchronize()
    ref = a.collect_synthetic(steps)
    assert torch.equal(act[:, :n], ref["action"]) and torch.equal(ob[:, :n], ref["ob"])
    assert torch.equal(rew[:, :n], ref["reward"]) and torch.equal(done[:, :n], ref["done_u8"])
    assert torch.equal(a.state, b.state)
    assert bool((act[:, n:] == -7).all()) and bool((ob[:, n:] == -7).all()) and bool((done[:, n:] == 9).all())
    bad = _native.lib().pomdp_collect_synthetic(
        _native.ENV_KIND[b.env_name], b._params_ref, b._state.data_ptr(), act.data_ptr(), ob.data_ptr(), rew.data_ptr(),
        done.data_ptr(), b._err.data_ptr(), n, b._seed, b.lane_offset, 0, steps, n - 4, _native.POMDP_AUTO_RESET, None)
    assert bad == -1                                        # POMDP_E_BADARG: pitch < n


@pytest.mark.parametrize("env,kw,auto,offset", [
    ("rock", {}, False, 0), ("rock", {}, True, 0), ("rock", dict(board_size=15, num_rocks=15), False, 0),
    ("rock", dict(board_size=15, num_rocks=15), True, 0), ("stochrock", {}, True, 0), ("stochrock", {}, False, 0),
    ("rock", {}, True, 1), ("network", {}, True, 0), ("network", {}, False, 0), ("network", dict(n_machines=31, problem_type=3), True, 0),
    ("network", {}, True, 2)],
    ids=["rock_7_8-frozen", "rock_7_8-auto", "rock_15_15-frozen", "rock_15_15-auto", "stochrock-auto", "stochrock-frozen",
         "rock_7_8-auto-actions_off_16_bytes", "network-auto", "network-frozen", "network_31-auto", "network-auto-actions_off_16_bytes"])
def test_step_contract_over_a_whole_2_20_batch(oracle_lib, env, kw, auto, offset):
    """env.step() at 2^20 lanes (step_quad_kernel / network_step_quad_kernel; with an action tensor that does not start on
    a 16-byte boundary the general step_kernel) against the oracle over the WHOLE batch, with caller-supplied actions of which a few are out of
    range and, without auto-reset, with lanes freezing as their episodes end."""
    n, seed, lane0 = 1 << 20, 606, 1 << 12
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, auto_reset=auto, reuse_buffers=True)
    o = oracle_lib.OracleEnv(env, **kw)
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, 0, nthreads=8))
    rs = np.random.RandomState(5)
    done = np.zeros(n, np.uint8)
    bad_total = 0
    for t in range(1, 9):
        a = rs.randint(o.n_actions, size=n).astype(np.int32)
        idx = rs.randint(n, size=2000)
        a[idx] = rs.choice([-1, o.n_actions, 1 << 20], size=len(idx))
        ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=auto, done=done, nthreads=8)
        bad_total += bad
        a_g = torch.zeros(n + offset, dtype=torch.int32, device="cuda")[offset:]
        a_g.copy_(torch.as_tensor(a))
        assert a_g.data_ptr() % 16 == 4 * offset
        ob_g, rew_g, done_g, _ = e.step(a_g)
        assert np.array_equal(np_(ob_g), ob) and np.array_equal(np_(rew_g), rew), t
        assert np.array_equal(np_(done_g), done.astype(bool)), t
        assert np.array_equal(np_(e.state).view(np.uint32), st), t
    assert e.invalid_action_count() == bad_total > 0


@pytest.mark.parametrize("env,kw", [("rock", {}), ("tag", {}), ("tiger", {}), ("battleship", {})],
                         ids=["rock", "tag", "tiger", "battleship"])
def test_collected_trajectories_do_not_depend_on_the_sharding(env, kw):
    """Lane sharding is exact for the fused launches too: the trajectories of lanes [0, 2^21) collected by one env equal
    those collected by two envs that own 2^20 lanes each (what two GPUs would do), row for row."""
    half, steps, seed = 1 << 20, 20, 8
    whole = make_env(env, kw, batch_size=2 * half, seed=seed)
    parts = [make_env(env, kw, batch_size=half, seed=seed, lane_offset=k * half) for k in range(2)]
    for e in [whole] + parts:
        e.reset()
    tw = whole.collect_synthetic(steps)
    for k, e in enumerate(parts):
        tp = e.collect_synthetic(steps)
        sl = slice(k * half, (k + 1) * half)
        for name in ("action", "ob", "reward", "done"):
            assert torch.equal(tw[name][:, sl], tp[name]), (env, k, name)
        assert torch.equal(whole.state[:, sl], e.state), (env, k)


def test_collect_into_columns_that_are_not_16_byte_aligned():
    """The quad-per-thread launches store 16 bytes at a time; columns that do not start on such a boundary (here: views one
    element into their allocations) must take the scalar path and give the same trajectories."""
    from gym_pomdp_amd import _native
    n, steps = 1 << 20, 18
    a = make_env("rock", {}, batch_size=n, seed=77, reuse_buffers=True)
    b = make_env("rock", {}, batch_size=n, seed=77, reuse_buffers=True)
    a.reset()
    b.reset()
    act = torch.zeros((steps + 1) * n + 1, dtype=torch.int32, device="cuda")[1:]
    ob = torch.zeros(steps * n + 1, dtype=torch.int32, device="cuda")[1:]
    rew = torch.zeros(steps * n + 1, dtype=torch.int32, device="cuda")[1:]
    done = torch.zeros(steps * n + 1, dtype=torch.uint8, device="cuda")[1:]
    assert act.data_ptr() % 16 == 4 and done.data_ptr() % 4 == 1
    rc = _native.lib().pomdp_collect_synthetic(
        _native.ENV_KIND["rock"], b._params_ref, b._state.data_ptr(), act.data_ptr(), ob.data_ptr(), rew.data_ptr(),
        done.data_ptr(), b._err.data_ptr(), n, b._seed, b.lane_offset, b._t, steps, n, _native.POMDP_AUTO_RESET, None)
    _native.check(rc, "pomdp_collect_synthetic")
    torch.cuda.synchronize()
    ref = a.collect_synthetic(steps)
    assert torch.equal(act.view(steps + 1, n), ref["action"]) and torch.equal(ob.view(steps, n), ref["ob"])
    assert torch.equal(rew.view(steps, n), ref["reward"]) and torch.equal(done.view(steps, n), ref["done_u8"])
    assert torch.equal(a.state, b.state)


@pytest.mark.parametrize("env,kw,how", [("rock", dict(use_heuristic=True), "heuristic"), ("tiger", {}, "heuristic"),
                                        ("tiger", {}, "rollout"), ("rock", {}, "rollout")],
                         ids=["rock-heuristic", "tiger-heuristic", "tiger-rollout", "rock-rollout"])
def test_scalar_env_keeps_stepping_through_the_c_side_drivers_after_a_reset(env, kw, how):
    """A batch_size=1 env whose episode ended inside heuristic_steps() / rollout_synthetic() — both take the DEVICE-side
    done flag as an in/out freeze flag — must be live again after reset(): lane L of a scalar env == lane L of a frozen
    batch (auto_reset=False; itself checked against the oracle above), call for call, across several resets."""
    from gym_pomdp_amd import History
    seed, lane0, n = 77, 4096, 64
    # a lane whose first episode is short (RockSample's heuristic policy can keep CHECKing for hundreds of steps): scout with
    # a frozen batch, then pair the scalar env with a batch that starts at that lane
    scout = make_env(env, kw, batch_size=1024, seed=seed, lane_offset=lane0, auto_reset=False)
    scout.reset()
    if how == "heuristic":
        scout.heuristic_steps(History(scout), 200)
    else:
        scout.rollout_synthetic(200)
    ended = torch.nonzero(scout._done.view(-1)[::4]).flatten() * 4     # ... on a quad boundary: the C-side drivers' shards start there
    assert len(ended) > 0
    lane0 += int(ended[0])
    pick = 0
    s = make_env(env, kw, seed=seed, lane_offset=lane0 + pick)
    b = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, auto_reset=False)
    assert s.reset() == int(b.reset()[pick])
    hs, hb = (History(s), History(b)) if how == "heuristic" else (None, None)
    resets = 0
    for i in range(1500):
        if how == "heuristic":
            outs_s, outs_b = s.heuristic_steps(hs, 1), b.heuristic_steps(hb, 1)
        else:
            outs_s, outs_b = s.rollout_synthetic(1), b.rollout_synthetic(1)
            outs_s = (s._action_scratch,) + tuple(outs_s)
            outs_b = (b._action_scratch,) + tuple(outs_b)
        row_s, row_b = [x[0].item() for x in outs_s], [x[pick].item() for x in outs_b]
        assert row_s == row_b, (env, how, i, row_s, row_b)
        assert torch.equal(s.state[:, 0], b.state[:, pick]), (env, how, i)
        if row_s[-1]:                                  # done: the reference's caller resets and goes on
            resets += 1
            assert s.reset() == int(b.reset()[pick])
            if how == "heuristic":
                hs, hb = History(s), History(b)
            if resets == 3:
                break
    assert resets >= 1, resets                         # (later episodes of the same lane may be long ones)


def test_collect_buffers_are_bound_per_env_and_per_buffer():
    """collect_synthetic caches the bound argument struct by the buffers' addresses ON THE ENV: a dict handed to a second
    env steps that env (not the first), replaced tensors are picked up, the dict holds tensors only, and a dict of the
    wrong shape is refused."""
    n, k = 4096, 12
    a = make_env("rock", {}, batch_size=n, seed=5, reuse_buffers=True)
    b = make_env("rock", {}, batch_size=n, seed=6, reuse_buffers=True)
    ref = make_env("rock", {}, batch_size=n, seed=6, reuse_buffers=True)
    for e in (a, b, ref):
        e.reset()
    tr = a.collect_synthetic(k)
    assert all(isinstance(v, torch.Tensor) for v in tr.values())
    state_a = a.state.clone()
    want = ref.collect_synthetic(k)
    got = b.collect_synthetic(k, out=tr)               # the same dict, another env
    assert torch.equal(a.state, state_a) and a.call_counter == 1 + k
    assert torch.equal(b.state, ref.state) and b.call_counter == 1 + k
    for name in ("action", "ob", "reward", "done"):
        assert torch.equal(got[name], want[name]), name
    # replaced tensors: the next call writes the new ones
    fresh = b.trajectory_buffers(k)
    old_ob = tr["ob"].clone()
    tr["ob"], tr["reward"] = fresh["ob"], fresh["reward"]
    want2 = ref.collect_synthetic(k)
    got2 = b.collect_synthetic(k, out=tr)
    assert torch.equal(got2["ob"], want2["ob"]) and torch.equal(got2["reward"], want2["reward"])
    assert got2["ob"].data_ptr() == fresh["ob"].data_ptr() and old_ob.shape == got2["ob"].shape
    with pytest.raises(ValueError):
        b.collect_synthetic(k + 1, out=tr)


def test_wide_integer_actions_never_wrap_into_valid_ones():
    """An int64 action such as 2^32 + 1 must not become action 1 through the int32 cast (the reference asserts on it,
    rock.py:125): it is counted invalid and the lane is left untouched, like any other out-of-range action."""
    n = 1024
    e = make_env("rock", {}, batch_size=n, seed=9)
    ref = make_env("rock", {}, batch_size=n, seed=9)
    e.reset()
    ref.reset()
    a64 = torch.ones(n, dtype=torch.int64, device="cuda")
    a64[::2] += 1 << 32                       # would wrap to the valid action 1
    a64[1] = -(1 << 32) + 2                   # would wrap to 2
    a32 = torch.where((a64 < 0) | (a64 >= e.action_space.n), torch.full_like(a64, -1), a64).to(torch.int32)
    ob, rew, done, _ = e.step(a64)
    ob2, rew2, done2, _ = ref.step(a32)
    assert torch.equal(ob, ob2) and torch.equal(rew, rew2) and torch.equal(done, done2) and torch.equal(e.state, ref.state)
    bad = int(((a64 < 0) | (a64 >= e.action_space.n)).sum())
    assert e.invalid_action_count() == ref.invalid_action_count() == bad == n // 2 + 1
    e.step(np.full(n, (1 << 32) + 3, dtype=np.int64))           # the numpy path
    assert e.invalid_action_count() == bad + n
    e.step(np.full(n, 3, dtype=np.uint8))
    assert e.invalid_action_count() == bad + n


def test_set_state_rejects_states_of_another_layout():
    """set_state / the planner hooks take int32 [state_words, N] only: a BattleShip state saved with 2 * MW words per lane
    (before the next-board contract) whose element count happens to divide by 3 * MW is not silently misread, and a
    hand-built state without a next board (its lanes could never finish a second episode) is rejected."""
    n = 96
    e = make_env("battleship", {}, batch_size=n, seed=1)
    e.reset()
    good = e.state.clone()
    assert e.state_words == 3
    with pytest.raises(ValueError):
        e.set_state(torch.zeros((2, n * 3 // 2), dtype=torch.int32))          # 2 * MW words per lane, same element count
    with pytest.raises(ValueError):
        e.set_state(good[:, : n // 2])
    empty_next = good.clone()
    empty_next[2] = 0
    with pytest.raises(ValueError):
        e.set_state(empty_next)
    e.set_state(good)
    assert torch.equal(e.state, good)
    r = make_env("rock", {}, batch_size=n, seed=1)
    r.reset()
    r.set_state(r.state.clone().reshape(-1))                                   # one-word layouts: [N] is unambiguous
    with pytest.raises(ValueError):
        r.legal_actions(torch.zeros((2, n), dtype=torch.int32))


def test_randomised_sweep_on_a_fixed_seed(monkeypatch):
    """tools/gpu_fuzz.py as part of the suite: 16 cases (the same on every machine: fixed seed, fixed count) of random env
    configs, batch sizes (both launch geometries), lane offsets up to 2^32, call counters up to 2^40, auto-reset on and off,
    invalid actions, and — one case in four here — trajectory collections in a random sink (columns / blocked / packed /
    narrow / returns-only), half of them on a random tape of caller's actions, each compared word for word with the
    oracle.  The builder's longer sweeps on fresh seeds are logged under profiles/."""
    import os
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    monkeypatch.setenv("FUZZ_COLLECT", "0.25")
    import gpu_fuzz
    assert gpu_fuzz.main(None, seed=20261001, n_cases=16) == 16


@pytest.mark.slow
def test_randomised_sweep_of_the_builders_long_run(monkeypatch):
    """The first 120 cases of the long sweep logged in profiles/r05_fuzz.txt (seed 777, one case in three a trajectory collection
    in a random sink — since round 6 half of those on a random tape of caller's actions): a fixed set, about a minute."""
    import os
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, "tools"))
    monkeypatch.setenv("FUZZ_COLLECT", "0.33")
    import gpu_fuzz
    assert gpu_fuzz.main(None, seed=777, n_cases=120) == 120
