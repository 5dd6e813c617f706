"""Particle beliefs on the GPU (pomdp_particle_init / pomdp_particle_update / pomdp_plan_particles, ParticleBelief,
plan(belief=) / plan_step(belief=)) against the contract's CPU restatement (tests/particle_restatement.py), bit for bit,
and what the filter means for Tiger, Tag and RockSample."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import particle_restatement as pr  # noqa: E402

pytestmark = pytest.mark.gpu

ENV_IDS = {"rock": "Rock-v0", "stochrock": "StochasticRock-v0", "tag": "Tag-v0", "battleship": "Battleship-v0", "tiger": "Tiger-v0",
           "network": "Network-v0"}
CASES = [("rock", {}), ("rock", dict(board_size=11, num_rocks=11)), ("rock", dict(board_size=15, num_rocks=15)), ("stochrock", {}),
         ("tag", {}), ("tag", dict(num_opponents=2)), ("tag", dict(num_opponents=3)), ("tag", dict(num_opponents=4)),
         ("battleship", {}), ("battleship", dict(board_size=(10, 10), max_len=5)), ("tiger", {}), ("network", {}),
         ("network", dict(n_machines=16, problem_type=2))]
IDS = ["%s%s" % (c[0], "-".join(str(v) for v in c[1].values())) for c in CASES]
SIZES = [(1, 4), (3, 64), (257, 256), (64, 4096)]
SEED = 4242


def np_(t):
    return t.detach().cpu().numpy()


def make(env, kw, n, **extra):
    import gym_pomdp_amd as gpa
    extra.setdefault("seed", SEED)
    extra.setdefault("auto_reset", False)
    return gpa.make(ENV_IDS[env], batch_size=n, **kw, **extra)


def u32(t):
    return np_(t).view(np.uint32)


def run_filter(env, kw, R, P, match_reward, use_done, steps=8, lane_offset=0, call_counter=0):
    """the real env under synthetic actions (auto_reset=False), a belief following it, and the restatement alongside;
    `call_counter`: the belief's call counter at its reset (the real env's own counter starts at 0 either way)"""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv(env, **kw)
    e = make(env, kw, R, lane_offset=lane_offset)
    b = e.particle_belief(P)
    b.call_counter = call_counter
    lane0 = lane_offset * P
    assert b.lane0 == lane0
    ob = e.reset()
    got = b.reset(ob)
    parts, nm = pr.init(o, None, R, P, b.seed, lane0, call_counter, ob=np.atleast_1d(np.asarray(ob if R == 1 else np_(ob))))
    nt = ol.max_threads()
    rs = np.random.RandomState(SEED)

    def actions():
        if lane_offset % 4:                                          # synthetic_actions() wants whole quads of lanes
            return torch.as_tensor(rs.randint(0, o.n_actions, R).astype(np.int32), device=e.device)
        return e.synthetic_actions()
    for t in range(call_counter + 1, call_counter + steps + 1):
        assert np.array_equal(u32(b.particles), parts), (env, kw, R, P, t)
        assert np.array_equal(np.atleast_1d(got if R == 1 else np_(got)), nm), (env, kw, R, P, t)
        if R == 1 and e.done:
            break                                                    # a single env asserts on a step after its episode ended
        a = actions() if R > 1 else int(actions().item())
        ob, rew, done, _ = e.step(a)
        tonp = (lambda x: np.atleast_1d(np.asarray(x))) if R == 1 else np_
        got = b.update(a, ob, rew if match_reward else None, done if use_done else None, match_reward=match_reward)
        parts, nm = pr.update(o, parts, tonp(a), tonp(ob), tonp(rew).astype(o.reward_dtype), tonp(done) if use_done else None,
                              match_reward, R, P, b.seed, lane0, t, nthreads=nt)
    assert np.array_equal(u32(b.particles), parts), (env, kw, R, P, "final")
    assert np.array_equal(np.atleast_1d(got if R == 1 else np_(got)), nm)
    assert b.call_counter == call_counter + steps + 1 or (R == 1 and e.done)
    return b, e


# The restatement's CPU time per case (reset + 8 updates, 8 threads, measured on the host): under 0.1 s at (1, 4) and (3, 64)
# but for a first call's thread start-up, 0.2 - 0.7 s at (257, 256), and at (64, 4096) 0.8 - 1.0 s for RockSample,
# StochasticRock and Tiger, 1.0 - 1.3 s for Tag, 1.2 - 1.5 s for Network, 1.5 s for BattleShip 5 x 5 and 2.0 s for 10 x 10;
# all 52 cases together 21 s.  Nothing is thinned: every env type runs at every size.
GRID = [(c, s) for c in range(len(CASES)) for s in SIZES]


@pytest.mark.parametrize("case,size", GRID, ids=["%s-%dx%d" % (IDS[c], s[0], s[1]) for c, s in GRID])
def test_filter_matches_the_restatement(case, size):
    env, kw = CASES[case]
    R, P = size
    combo = (case + SIZES.index(size)) % 4
    run_filter(env, kw, R, P, match_reward=combo & 1 == 1, use_done=combo & 2 == 2)


# The shapes at which particle_kernel's index arithmetic branches, (R, P); R leaves the last workgroup partial where a
# workgroup holds G = 256 // P > 1 roots.
GEOMETRY = [(43, 12), (5, 100), (3, 252),          # narrow, P does not divide 256: G = 21 / 2 / 1, 4 / 56 / 4 idle tail threads
            (33, 8), (3, 128),                      # narrow, P divides 256
            (5, 512), (3, 2048),                    # wide, whole chunks
            (3, 260), (5, 1000), (2, 4092)]         # wide, ragged last chunk (260: 4 slots in chunk 1)
# The restatement's CPU time per case at these shapes (measured as above): 0.00 - 0.15 s each but for thread start-up, the
# 13 x 10 cases together 6 s.  Nothing is thinned: every env type runs at every row.
GEOGRID = [(c, s) for c in range(len(CASES)) for s in GEOMETRY]


@pytest.mark.parametrize("case,size", GEOGRID, ids=["%s-%dx%d" % (IDS[c], s[0], s[1]) for c, s in GEOGRID])
def test_filter_matches_the_restatement_at_every_geometry(case, size):
    """Bit for bit like test_filter_matches_the_restatement, at the narrow shapes whose roots start and end inside a ballot
    word or leave idle threads, and at the wide shapes with several chunks, whole or ragged.  The match_reward / use_done
    combination rotates with the case, so every row sees all four."""
    env, kw = CASES[case]
    R, P = size
    combo = (case + GEOMETRY.index(size)) % 4
    run_filter(env, kw, R, P, match_reward=combo & 1 == 1, use_done=combo & 2 == 2)


# lane offsets and call counters: (R, P) of one narrow row whose P does not divide 256, one wide ragged row and P = 4096
EDGE_ROWS = [(43, 12), (5, 1000), (64, 4096)]
EDGE_KEYS = {"top-lanes": None, "t-crosses-2^32": (1 << 32) - 3, "t-past-2^33": (1 << 33) + 1}


@pytest.mark.parametrize("how", list(EDGE_KEYS))
@pytest.mark.parametrize("size", EDGE_ROWS, ids=["%dx%d" % s for s in EDGE_ROWS])
@pytest.mark.parametrize("env", ["rock", "tag", "battleship"])
def test_filter_at_the_last_lanes_and_past_32_bit_call_counters(env, size, how):
    """top-lanes: lane_offset = 2^32 // P - R, the last roots a belief of P particles can hold (P = 4096, R = 64: lane0 +
    R * P == 2^32 exactly, the last particle is global lane 0xFFFFFFFF).  The others: the belief's call counter starts at
    2^32 - 3 (the high counter word changes between the third and the fourth update) or at 2^33 + 1."""
    R, P = size
    combo = (EDGE_ROWS.index(size) + list(EDGE_KEYS).index(how)) % 4
    if EDGE_KEYS[how] is None:
        off = (1 << 32) // P - R
        assert (1 << 32) - P < (off + R) * P <= 1 << 32
        run_filter(env, {}, R, P, combo & 1 == 1, combo & 2 == 2, lane_offset=off)
    else:
        run_filter(env, {}, R, P, combo & 1 == 1, combo & 2 == 2, call_counter=EDGE_KEYS[how])


@pytest.mark.parametrize("match_reward", [False, True])
@pytest.mark.parametrize("use_done", [False, True])
def test_filter_matching_options_rock(match_reward, use_done):
    run_filter("rock", {}, 257, 256, match_reward, use_done)
    run_filter("tag", {}, 3, 64, match_reward, use_done)


@pytest.mark.parametrize("P", [64, 100, 260, 1024])
def test_edge_roots_depleted_out_of_range_and_masked_init(P):
    from oracle import oracle_lib as ol
    R = 40
    o = ol.OracleEnv("rock")
    e = make("rock", {}, R)
    b = e.particle_belief(P)
    ob = np_(e.reset())
    b.reset(ob)
    parts, _ = pr.init(o, None, R, P, b.seed, 0, 0, ob=ob)
    a = np_(e.synthetic_actions()).copy()
    ob1, rew, done, _ = e.step(torch.as_tensor(a, device=e.device))
    ob1 = np_(ob1).copy()
    ob1[::5] = -5                                                   # no particle observes -5: depleted, left unfiltered
    a[1::7] = -1                                                    # a plan's best == -1
    a[2::7] = o.n_actions                                           # out of range
    before = u32(b.particles).copy()
    nm = np_(b.update(a, ob1)).copy()
    want, wnm = pr.update(o, parts, a, ob1, None, None, False, R, P, b.seed, 0, 1)
    assert np.array_equal(u32(b.particles), want) and np.array_equal(nm, wnm)
    bad = (a < 0) | (a >= o.n_actions)
    assert (nm[bad] == -1).all()
    assert np.array_equal(u32(b.particles).reshape(-1, R, P)[:, bad], before.reshape(-1, R, P)[:, bad])
    dep = (np.arange(R) % 5 == 0) & ~bad
    assert (nm[dep] == 0).all() and np.array_equal(np_(b.depleted), nm == 0)
    # init with a mask: the masked roots start over, the others are left untouched
    where = np.arange(R) % 3 == 0
    cur = u32(b.particles).copy()
    ob2 = np_(e.reset(where=torch.as_tensor(where, device=e.device)))
    nm2 = np_(b.reset(ob2, where=where)).copy()
    want2, wnm2 = pr.init(o, cur, R, P, b.seed, 0, 2, ob=ob2, where=where)
    assert np.array_equal(u32(b.particles), want2) and np.array_equal(nm2, wnm2)
    assert (nm2[~where] == -1).all() and (nm2[where] == P).all()


def test_sharded_beliefs_equal_one_belief():
    R, P = 96, 128
    # every shard takes the whole batch's actions of its own lanes
    whole = make("tag", {}, R)
    halves = [make("tag", {}, R // 2, lane_offset=k * R // 2) for k in range(2)]
    bw = whole.particle_belief(P)
    bh = [h.particle_belief(P) for h in halves]
    bw.reset(whole.reset())
    for h, b in zip(halves, bh):
        b.reset(h.reset())
    for _ in range(6):
        a = whole.synthetic_actions()
        ow, rw, dw, _ = whole.step(a)
        nmw = np_(bw.update(a, ow, rw, dw, match_reward=True)).copy()
        nmh = []
        for k, (h, b) in enumerate(zip(halves, bh)):
            ak = a[k * R // 2:(k + 1) * R // 2].contiguous()
            oh, rh, dh, _ = h.step(ak)
            nmh.append(np_(b.update(ak, oh, rh, dh, match_reward=True)).copy())
        assert np.array_equal(nmw, np.concatenate(nmh))
        assert np.array_equal(u32(bw.particles), np.concatenate([u32(b.particles) for b in bh], axis=1))
    pw = whole.plan(6, sims_per_root=256, belief=bw)
    ph = [h.plan(6, sims_per_root=256, belief=b) for h, b in zip(halves, bh)]
    for k in ("q", "visits", "best"):
        assert np.array_equal(np_(pw[k]), np.concatenate([np_(p[k]) for p in ph])), k


@pytest.mark.parametrize("env,kw,R,P,S", [("rock", {}, 64, 64, 256), ("rock", dict(board_size=15, num_rocks=15), 33, 32, 96),
                                          ("tag", {}, 16, 256, 512), ("tiger", {}, 8, 4, 64), ("battleship", {}, 5, 16, 64),
                                          ("rock", {}, 7, 100, 300), ("rock", {}, 5, 260, 520)])
def test_plan_from_particles_matches_the_restatement(env, kw, R, P, S):
    from oracle import oracle_lib as ol
    o = ol.OracleEnv(env, **kw)
    e = make(env, kw, R, lane_offset=4)
    b = e.particle_belief(P)
    b.reset(e.reset())
    a = e.synthetic_actions()
    ob, rew, done, _ = e.step(a)
    b.update(a, ob, rew, done)
    parts = u32(b.particles).copy()
    t0 = e.call_counter
    got = e.plan(10, sims_per_root=S, belief=b)
    want, sims = pr.plan(o, parts, R, P, S, 10, e._discount, e._seed, 4 * S, t0, nthreads=ol.max_threads())
    assert np.array_equal(np_(got["q"]).view(np.uint64), want["q"].view(np.uint64))
    assert np.array_equal(np_(got["visits"]), want["visits"]) and np.array_equal(np_(got["best"]), want["best"])
    assert np.array_equal(np_(got["sim_ret"]).view(np.uint64), sims["ret"].view(np.uint64))
    with pytest.raises(ValueError):
        e.plan(10, sims_per_root=S + 2, belief=b)
    other = make(env, kw, R + 1)
    with pytest.raises(ValueError):
        other.plan(10, sims_per_root=S, belief=b)


def test_plan_step_keeps_env_and_belief_consistent():
    """16 planned steps of RockSample(7,8), 1024 roots x 256 particles, 256 simulations per root: the env's state, the
    belief and every plan equal the restatement driving the oracle with the restated plans' actions."""
    from oracle import oracle_lib as ol
    R, P, S, depth = 1024, 256, 256, 8
    o = ol.OracleEnv("rock")
    nt = ol.max_threads()
    e = make("rock", {}, R)
    b = e.particle_belief(P)
    real = o.new_state(R)
    ob = e.reset()
    assert np.array_equal(np_(ob), o.batch_reset(real, SEED, 0, 0, nthreads=nt))
    b.reset(ob)
    parts, _ = pr.init(o, None, R, P, b.seed, 0, 0, ob=np_(ob))
    done = np.zeros(R, np.uint8)
    e2 = make("rock", {}, 8, auto_reset=True)
    with pytest.raises(ValueError):                                  # an auto-reset step would hide the fresh episode's observation
        e2.plan_step(depth, S, belief=e2.particle_belief(P))
    for k in range(16):
        t0 = e.call_counter
        ob, rew, dn, _, plan = e.plan_step(depth, sims_per_root=S, belief=b)
        want, _ = pr.plan(o, parts, R, P, S, depth, e._discount, SEED, 0, t0, nthreads=nt)
        assert np.array_equal(np_(plan["best"]), want["best"]), k
        assert np.array_equal(np_(plan["q"]).view(np.uint64), want["q"].view(np.uint64)), k
        ob_o, rew_o, done, _ = o.batch_step(real, want["best"], SEED, 0, t0 + depth, auto_reset=False, done=done, nthreads=nt)
        assert np.array_equal(np_(ob), ob_o) and np.array_equal(np_(rew), rew_o) and np.array_equal(np_(dn), done.astype(bool))
        assert np.array_equal(u32(e.state), real), k
        parts, nm = pr.update(o, parts, want["best"], ob_o, rew_o, done, False, R, P, b.seed, 0, k + 1, nthreads=nt)
        assert np.array_equal(u32(b.particles), parts) and np.array_equal(np_(b.n_match), nm), k


def test_tiger_posterior_on_the_gpu():
    """The host test's Bayes check, on the HIP path: Tiger roots LISTEN eight times; the fraction of particles with the tiger
    behind the left door (state bit 0 == 0) follows .85^L .15^R / (.85^L .15^R + .15^L .85^R)."""
    R, P = 1024, 256
    e = make("tiger", {}, R, seed=91)
    b = e.particle_belief(P)
    b.reset(e.reset())
    n_left = torch.zeros(R, dtype=torch.int64, device=e.device)
    listen = torch.full((R,), 2, dtype=torch.int32, device=e.device)
    for _ in range(8):
        ob, rew, done, _ = e.step(listen)
        n_left += (ob == 0).long()
        b.update(listen, ob, rew, done, match_reward=True)
        assert (np_(b.n_match) >= 1).all()
    L = np_(n_left)
    frac = ((np_(b.particles)[0].reshape(R, P) & 1) == 0).mean(axis=1)
    checked = 0
    for l in np.unique(L):
        sel = L == l
        if sel.sum() < 20:
            continue
        post = .85 ** l * .15 ** (8 - l) / (.85 ** l * .15 ** (8 - l) + .15 ** l * .85 ** (8 - l))
        se = np.sqrt(post * (1 - post) / (sel.sum() * P)) + frac[sel].std() / np.sqrt(sel.sum())
        assert abs(frac[sel].mean() - post) < 4.5 * se + 0.01, (l, frac[sel].mean(), post)
        checked += 1
    assert checked >= 3


def test_tag_survivors_stand_on_the_observed_cell():
    R, P = 512, 256
    e = make("tag", {}, R, seed=5)
    b = e.particle_belief(P)
    b.reset(e.reset())
    for _ in range(8):
        a = e.synthetic_actions()
        ob, rew, done, _ = e.step(a)
        nm = np_(b.update(a, ob, rew, done))
        agent = (np_(b.particles)[0].reshape(R, P) & 31)
        seen = (np_(ob) < 29) & (nm >= 1)
        assert seen.sum() > R // 4
        assert (agent[seen] == np_(ob)[seen][:, None]).all()


def test_rock_check_at_distance_zero_settles_the_rock():
    """An agent on rock 0's cell CHECKs it: the sensor's efficiency is 1 at distance 0, so every survivor agrees with the
    real rock's status."""
    R, P = 256, 256
    e = make("rock", {}, R, seed=8)
    b = e.particle_belief(P)
    b.reset(e.reset())
    pos = int(e._params.rock_x[0]) | (int(e._params.rock_y[0]) << 4)
    st = np_(e.state).copy()
    st[0] = (st[0] & ~0xFF) | pos
    e.set_state(torch.as_tensor(st, device=e.device))
    pt = np_(b.particles).copy()
    pt[0] = (pt[0] & ~0xFF) | pos
    b.set_particles(torch.as_tensor(pt, device=e.device))
    a = torch.full((R,), 5, dtype=torch.int32, device=e.device)          # CHECK rock 0
    ob, rew, done, _ = e.step(a)
    nm = np_(b.update(a, ob, rew, done))
    assert (nm >= 1).all()
    status = (np_(b.particles)[0].reshape(R, P) >> 8) & 3
    real = (np_(e.state)[0] >> 8) & 3
    assert (status == real[:, None]).all()


def test_c_abi_directly():
    """pomdp_particle_init / _update through ctypes, without the Python class."""
    from gym_pomdp_amd import _native
    from oracle import oracle_lib as ol
    L = _native.lib()
    R, P, seed = 7, 32, 1234
    e = make("tiger", {}, R)
    o = ol.OracleEnv("tiger")
    parts = torch.zeros((1, R * P), dtype=torch.int32, device=e.device)
    out = torch.zeros_like(parts)
    nm = torch.zeros(R, dtype=torch.int32, device=e.device)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.pomdp_particle_init(_native.ENV_KIND["tiger"], e._params_ref, parts.data_ptr(), None, None, nm.data_ptr(), R, P, seed,
                                 0, 0, stream) == 0
    want, wnm = pr.init(o, None, R, P, seed, 0, 0)
    assert np.array_equal(u32(parts), want) and np.array_equal(np_(nm), wnm)
    act = torch.full((R,), 2, dtype=torch.int32, device=e.device)
    ob = torch.tensor([0, 1, 0, 1, 0, 1, 2], dtype=torch.int32, device=e.device)
    assert L.pomdp_particle_update(_native.ENV_KIND["tiger"], e._params_ref, parts.data_ptr(), out.data_ptr(), act.data_ptr(),
                                   ob.data_ptr(), None, None, nm.data_ptr(), R, P, 0, seed, 0, 1, stream) == 0
    want2, wnm2 = pr.update(o, want, np_(act), np_(ob), None, None, False, R, P, seed, 0, 1)
    assert np.array_equal(u32(out), want2) and np.array_equal(np_(nm), wnm2)
    assert np_(nm)[6] == 0                                               # LISTEN never observes 2
    assert L.pomdp_particle_update(_native.ENV_KIND["tiger"], e._params_ref, parts.data_ptr(), parts.data_ptr(), act.data_ptr(),
                                   ob.data_ptr(), None, None, nm.data_ptr(), R, P, 0, seed, 0, 1, stream) == -1


def test_batch_of_one_takes_python_ints():
    R, P = 1, 64
    e = make("rock", {}, R)
    b = e.particle_belief(P)
    assert b.reset(e.reset()) == P
    ob, rew, done, _ = e.step(1)
    n = b.update(1, ob, rew, done, match_reward=True)
    assert isinstance(n, int) and 1 <= n <= P
    assert b.seed != e._seed


# ---- constructed survivor sets -----------------------------------------------------------------------------------------------
SURVIVOR_SETS = {"slot0": lambda P: [0], "slot63": lambda P: [63], "slot64": lambda P: [64], "last": lambda P: [P - 1],
                 "all": lambda P: list(range(P)), "none": lambda P: [], "every65th": lambda P: list(range(0, P, 65)),
                 "ragged-chunk": lambda P: list(range(P - P % 256, P))}
SURVIVOR_CASES = [(P, k) for P in (100, 256, 260, 4096) for k in SURVIVOR_SETS if k != "ragged-chunk" or P == 260]


def survivor_particles(real, P, names):
    """RockSample(7,8) particles for roots whose agent stands on rock 0's cell and CHECKs it: slot j of root r carries the
    real state's position, rocks 1..7 good / bad after the bits of j % 128 (so that a copy from the wrong survivor shows) and
    rock 0 like the real state's iff j is in the root's survivor set `names[r]`, the other way round otherwise."""
    R = len(real)
    j = np.arange(P, dtype=np.uint32)
    pattern = sum(((j >> i) & 1) << (11 + 2 * i) for i in range(7)).astype(np.uint32)      # code 2 (good) or 0 (bad)
    parts = np.zeros((R, P), np.uint32)
    for r in range(R):
        code = (real[r] >> 8) & 3
        assert code in (0, 2)
        surv = np.zeros(P, bool)
        surv[SURVIVOR_SETS[names[r]](P)] = True
        parts[r] = (real[r] & 0xFF) | pattern | (np.where(surv, code, 2 - code).astype(np.uint32) << 8)
    return parts.reshape(1, R * P)


@pytest.mark.parametrize("P,first", SURVIVOR_CASES, ids=["%d-%s" % c for c in SURVIVOR_CASES])
def test_constructed_survivor_sets(P, first):
    """The survivor list's corners.  The sensor is exact at distance 0, so a particle survives iff its rock 0 agrees with the
    real one, and a CHECK leaves the state as it is: the proposals are the particles set.  Root r takes the survivor set
    that follows `first` by r places, so the roots of one launch (and the neighbours inside a narrow workgroup: P = 100 puts
    "all" next to "none") differ; 2 * sets + 1 roots leave the last narrow workgroup partial."""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("rock")
    keys = [k for p, k in SURVIVOR_CASES if p == P]
    R = 2 * len(keys) + 1
    names = [keys[(keys.index(first) + r) % len(keys)] for r in range(R)]
    e = make("rock", {}, R, seed=8)
    b = e.particle_belief(P)
    b.reset(e.reset())
    pos = int(e._params.rock_x[0]) | (int(e._params.rock_y[0]) << 4)
    st = np_(e.state).copy()
    st[0] = (st[0] & ~0xFF) | pos
    e.set_state(torch.as_tensor(st, device=e.device))
    parts = survivor_particles(st[0].view(np.uint32), P, names)
    assert ((parts & 15) < 7).all() and (((parts >> 4) & 15) < 7).all() and ((parts >> 24) == 0).all()   # what set_particles checks
    assert (((parts >> 8) & 0x5555) == 0).all()                      # every rock good (2) or bad (0)
    b.set_particles(torch.as_tensor(parts.view(np.int32), device=e.device))
    a = torch.full((R,), 5, dtype=torch.int32, device=e.device)     # CHECK rock 0
    ob, rew, done, _ = e.step(a)
    nm = np_(b.update(a, ob)).copy()
    want, wnm = pr.update(o, parts, np_(a), np_(ob), None, None, False, R, P, b.seed, 0, 1)
    got = u32(b.particles)
    assert np.array_equal(got, want) and np.array_equal(nm, wnm)
    for r in range(R):
        slots = SURVIVOR_SETS[names[r]](P)
        root, was = got[0, r * P:(r + 1) * P], parts[0, r * P:(r + 1) * P]
        assert nm[r] == len(slots), (r, names[r])
        if len(slots) == 1:
            assert (root == was[slots[0]]).all(), (r, names[r])
        elif len(slots) in (0, P):
            assert np.array_equal(root, was), (r, names[r])
        else:
            assert np.isin(root, was[slots]).all() and np.array_equal(root[slots], was[slots]), (r, names[r])


def test_rock_one_check_gives_the_exact_posterior_on_the_gpu():
    """test_particles_host's one-step posterior check (see there, also for why it stops at one update) through ParticleBelief:
    RockSample(7,8), 4096 roots x 252 particles, root r CHECKs rock r % 8 from the reset prior; bound: five standard errors."""
    from oracle import oracle_lib as ol
    from test_particles_host import rock_check_posterior
    R, P = 4096, 252
    o = ol.OracleEnv("rock")
    e = make("rock", {}, R, seed=5)
    b = e.particle_belief(P, seed=11)
    assert (np_(b.reset(e.reset())) == P).all()
    a = torch.as_tensor((5 + np.arange(R) % 8).astype(np.int32), device=e.device)
    ob, rew, done, _ = e.step(a)
    nm = np_(b.update(a, ob)).copy()
    rock_check_posterior(o, u32(e.state), np_(a), np_(ob), u32(b.particles), nm, P, min_groups=10)


def test_c_abi_at_the_last_lane_and_one_past_it():
    """pomdp_particle_init / _update through ctypes with lane0 = 2^32 - R * P for P = 1000, which is no multiple of P (no
    lane_offset of an env gives it): the last particle is global lane 0xFFFFFFFF.  Four lanes further the call is refused
    and nothing is launched."""
    from gym_pomdp_amd import _native
    from oracle import oracle_lib as ol
    L = _native.lib()
    R, P, seed = 5, 1000, 1234
    lane0 = (1 << 32) - R * P
    assert lane0 % 4 == 0 and lane0 % P
    e = make("rock", {}, R)
    o = ol.OracleEnv("rock")
    kind = _native.ENV_KIND["rock"]
    parts = torch.zeros((1, R * P), dtype=torch.int32, device=e.device)
    out = torch.zeros_like(parts)
    nm = torch.zeros(R, dtype=torch.int32, device=e.device)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.pomdp_particle_init(kind, e._params_ref, parts.data_ptr(), None, None, nm.data_ptr(), R, P, seed, lane0, 0, stream) == 0
    want, wnm = pr.init(o, None, R, P, seed, lane0, 0)
    assert np.array_equal(u32(parts), want) and np.array_equal(np_(nm), wnm)
    act = torch.tensor([5, 6, 7, 8, 12], dtype=torch.int32, device=e.device)                  # CHECK rocks 0, 1, 2, 3, 7
    ob = torch.tensor([1, 2, 1, 2, 0], dtype=torch.int32, device=e.device)                    # a CHECK never observes 0
    assert L.pomdp_particle_update(kind, e._params_ref, parts.data_ptr(), out.data_ptr(), act.data_ptr(), ob.data_ptr(), None, None,
                                   nm.data_ptr(), R, P, 0, seed, lane0, 1, stream) == 0
    want2, wnm2 = pr.update(o, want, np_(act), np_(ob), None, None, False, R, P, seed, lane0, 1)
    assert np.array_equal(u32(out), want2) and np.array_equal(np_(nm), wnm2)
    assert (wnm2[:4] >= 1).all() and (wnm2[:4] < P).all() and wnm2[4] == 0
    out.fill_(-1)
    nm.fill_(-7)
    assert L.pomdp_particle_init(kind, e._params_ref, out.data_ptr(), None, None, nm.data_ptr(), R, P, seed, lane0 + 4, 0, stream) == -1
    assert L.pomdp_particle_update(kind, e._params_ref, parts.data_ptr(), out.data_ptr(), act.data_ptr(), ob.data_ptr(), None, None,
                                   nm.data_ptr(), R, P, 0, seed, lane0 + 4, 1, stream) == -1
    torch.cuda.synchronize()
    assert (np_(out) == -1).all() and (np_(nm) == -7).all()
