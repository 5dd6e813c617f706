"""Stochastic finite-state controllers inside the fused loop (env.run_controller(StochasticController),
pomdp_stoch_controller_episodes) against the contract's CPU restatement (tests/stoch_controller_restatement.py: the oracle
stepped with auto_reset=False, the draws from oracle.philox_ref), bit for bit: records, node, state, done, the
invalid_action_count() delta and the returns statistics.  The restatement reads the thresholds the controller holds, so the host
class's quantisation is not part of the comparison (test_stoch_controller_host.py checks it)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoch_controller_restatement as sr  # noqa: E402
from test_gpu_controller import ENV_IDS, STEPS  # noqa: E402
from test_stoch_controller_host import FREQ_N, FREQ_P, FREQ_SEED, frequency_case, within_five_sigma  # noqa: E402

pytestmark = pytest.mark.gpu

N, LANE0, SEED = 1000, 8, 12345       # three full workgroups, a partial one and a ragged last wave


def np_(t):
    return t.detach().cpu().numpy()


def u32(t):
    return np_(t).view(np.uint32)


def rows_of(out, k, n):
    """the packed records uint32 [k, n] of a packed or narrow trajectory"""
    if out["layout"] == "packed":
        return np_(out["traj"][:k, :n]).view(np.uint32)
    t = np_(out["traj"][:k, :, :n]).astype(np.uint32)
    return t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16) | (t[:, 3] << 24)


def same_f64(got, want):
    """bit for bit; the NaN a fresh ret_done holds equals itself"""
    return bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def random_tables(o, K=7, B=3, D=2, seed=7, n=N):
    """a seeded random controller in candidate form — (action, action_p, next, next_p) — and per-lane random start nodes"""
    rng = np.random.RandomState(seed)
    ap, nxp = rng.uniform(.05, 1.0, (K, B)), rng.uniform(.05, 1.0, (K, o.n_obs, D))
    return (rng.randint(0, o.n_actions, (K, B)), ap / ap.sum(-1, keepdims=True), rng.randint(0, K, (K, o.n_obs, D)),
            nxp / nxp.sum(-1, keepdims=True)), rng.randint(0, K, n)


class Run(object):
    """one env on the GPU and the oracle after the same reset() (call counter 0), and a controller of the GPU env built by
    make_ctrl(env); the restatement runs on the tables and thresholds that controller holds"""

    def __init__(self, ol, env, make_ctrl, n=N, lane0=LANE0, seed=SEED, **kw):
        import gym_pomdp_amd as gpa
        self.ol, self.env, self.nt, self.n, self.lane0, self.seed = ol, env, ol.max_threads(), n, lane0, seed
        self.o = ol.OracleEnv(env, **kw)
        self.e = gpa.make(ENV_IDS[env], batch_size=n, seed=seed, lane_offset=lane0, auto_reset=False, **kw)
        self.st0 = self.o.new_state(n)
        ob = self.o.batch_reset(self.st0, seed, lane0, 0, nthreads=self.nt)
        assert np.array_equal(np_(self.e.reset()), ob)
        self.gpu_st0 = self.e._state.clone()
        self.ctrl = make_ctrl(self.e)
        self.start = np_(self.ctrl.node).astype(np.int64)
        self.tables = (np_(self.ctrl.action).astype(np.int64), u32(self.ctrl.action_thr), np_(self.ctrl.next).astype(np.int64),
                       u32(self.ctrl.next_thr))

    def reference(self, k, calls=1, done0=None):
        """[(packed, refused entries so far, state, done, node, acc, cnt)] after each of `calls` calls of k steps from t = 1"""
        st, node = self.st0.copy(), self.start.copy()
        done = np.zeros(self.n, np.uint8) if done0 is None else done0.copy()
        acc, cnt = self.ol.new_return_stats(self.n)
        res, bad = [], 0
        for c in range(calls):
            packed, b = sr.run(self.o, st, done, node, *self.tables, k, self.seed, self.lane0, 1 + c * k, acc, cnt,
                               float(self.e._discount), nthreads=self.nt)
            bad += b
            res.append((packed, bad, st.copy(), done.copy(), node.copy(), acc.copy(), cnt.copy()))
        return res

    def rewind(self, done0=None):
        """back to the state after reset(): call counter 1, nobody done (or done0), every lane on its start node, nothing counted"""
        self.e._state.copy_(self.gpu_st0)
        self.e._done.zero_()
        if done0 is not None:
            self.e._done.copy_(torch.as_tensor(done0, device=self.e.device))
        self.e._err.zero_()
        self.e.call_counter = 1
        self.ctrl.node.copy_(torch.as_tensor(self.start.astype(np.int32), device=self.e.device))

    def check(self, k, ref, layouts=("packed", "narrow", "returns"), done0=None):
        """run_controller, once per entry of `ref` in a row (out / stats continued), in every layout, against `ref`"""
        from gym_pomdp_amd import _native
        n = self.n
        for layout in layouts:
            self.rewind(done0)
            res = None
            for c, (packed, bad, st, done, node, acc, cnt) in enumerate(ref):
                ctx = (self.env, layout, c)
                if layout == "returns":
                    res = self.e.run_controller(self.ctrl, k, stats=res)
                    assert same_f64(np_(res.acc[:, :n]), acc), ctx
                    assert np.array_equal(np_(res.cnt[:, :n]), cnt), ctx
                else:
                    res = self.e.run_controller(self.ctrl, k, layout=layout, out=res)
                    got = rows_of(res, k, n)
                    assert np.array_equal(got, packed), ctx + (np.argwhere(got != packed)[:4].tolist(),)
                assert _native.lib().pomdp_last_fused_kernel().decode().startswith("stoch_controller_kernel<"), ctx
                assert np.array_equal(np_(self.e.state).view(np.uint32), st), ctx
                assert np.array_equal(np_(self.e._done), done) and torch.equal(self.e.done, self.e._done.view(torch.bool)), ctx
                assert np.array_equal(np_(self.ctrl.node), node), ctx
                assert self.e.invalid_action_count() == bad, ctx
                assert self.e.call_counter == 1 + (c + 1) * k, ctx


def stoch(tables, start, **kw):
    """make_ctrl of a StochasticController on (action, action_p, next, next_p)"""
    import gym_pomdp_amd as gpa
    return lambda e: gpa.StochasticController(e, *tables, start=start, **kw)


def raw(action, action_thr, nxt, next_thr, start):
    """make_ctrl of an unvalidated StochasticController on raw thresholds"""
    import gym_pomdp_amd as gpa
    return lambda e: gpa.StochasticController(e, action, None, nxt, None, start=start, validate=False, action_thr=action_thr,
                                              next_thr=next_thr)


# ---- 1. every env form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", list(STEPS))
def test_two_calls_in_a_row_equal_the_restatement(oracle_lib, env):
    """K = 7, B = 3, D = 2; packed rows, narrow rows, returns statistics, final state, done, node and the count after each of two
    calls in a row: the second starts with frozen lanes and carried nodes.
    The share of lanes the first call finishes (from the restatement, exactly this setup): rock 0.56, stochrock 0.012, tag 0.09,
    tiger 0.97, battleship 0.010 — neither an all-live nor an all-frozen batch; Network's episodes never end."""
    k = STEPS[env]
    tables, start = random_tables(oracle_lib.OracleEnv(env), seed=10)
    r = Run(oracle_lib, env, stoch(tables, start))
    ref = r.reference(k, calls=2)
    finished = float(ref[0][3].astype(bool).mean())
    print("%s: share of lanes finished by the first call %.3f" % (env, finished))
    if env != "network":
        assert 0 < finished < 1, finished
    assert ref[1][1] == 0
    r.check(k, ref)


# ---- 2. one candidate each: the deterministic loop -------------------------------------------------------------------------------
@pytest.mark.parametrize("env", list(STEPS))
def test_one_candidate_each_equals_the_deterministic_loop(oracle_lib, env):
    """B = D = 1 (from_controller): records, node, state, done and statistics are those of run_controller(Controller(...)) on
    the same env and seed"""
    import gym_pomdp_amd as gpa
    k = STEPS[env]
    o = oracle_lib.OracleEnv(env)
    rng = np.random.RandomState(7)
    action, nxt, start = rng.randint(0, o.n_actions, 128), rng.randint(0, 128, (128, o.n_obs)), rng.randint(0, 128, N)
    e = gpa.make(ENV_IDS[env], batch_size=N, seed=SEED, lane_offset=LANE0, auto_reset=False)
    e.reset()
    st0 = e._state.clone()
    det = gpa.Controller(e, action, nxt, start=start)
    sto = gpa.StochasticController.from_controller(det)
    got = []
    for ctrl in (det, sto):
        res = []
        for layout in ("packed", "returns"):
            e._state.copy_(st0)
            e._done.zero_()
            e.call_counter = 1
            ctrl.reset_nodes()
            out = e.run_controller(ctrl, k, layout=layout)
            res += [rows_of(out, k, N)] if layout == "packed" else [np_(out.acc).view(np.uint64), np_(out.cnt)]
            res += [np_(e.state), np_(e._done), np_(ctrl.node)]
        got.append(res)
    assert e.invalid_action_count() == 0
    for x, y in zip(*got):
        assert np.array_equal(x, y)


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["rock", "tag"])
def test_results_do_not_depend_on_the_steps_per_launch(oracle_lib, env):
    """ten steps with pomdp_fuse_max 4 (launches of 4 + 4 + 2, the node carried from one to the next) and then 256"""
    from gym_pomdp_amd import _native
    L = _native.lib()
    k = 10
    tables, start = random_tables(oracle_lib.OracleEnv(env))
    r = Run(oracle_lib, env, stoch(tables, start))
    got = {}
    old = L.pomdp_fuse_max(0)
    try:
        for fuse in (4, 256):
            L.pomdp_fuse_max(fuse)
            r.rewind()
            rows = rows_of(r.e.run_controller(r.ctrl, k, layout="packed"), k, N)
            res = [rows, np_(r.e.state), np_(r.e._done), np_(r.ctrl.node)]
            r.rewind()
            stats = r.e.run_controller(r.ctrl, k)
            got[fuse] = res + [np_(stats.acc), np_(stats.cnt), np_(r.e.state), np_(r.ctrl.node)]
    finally:
        L.pomdp_fuse_max(old)
    for x, y in zip(got[4], got[256]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(got[4][0], r.reference(k)[0][0])


# ---- 4. the pick rule's edges ----------------------------------------------------------------------------------------------------
LISTEN, OPEN0 = 2, 0


@pytest.mark.parametrize("which", ["action", "next"])
def test_a_threshold_at_below_and_above_the_lanes_own_word(oracle_lib, which):
    """Tiger, 64 lanes, K = 3 * 64: lane i's nodes 3 i + j carry the threshold u, u - 1 and u + 1 (j = 0, 1, 2) of ITS OWN step-0
    draw u — u_a in action_thr, u_n in next_thr.  The compare is strict: u > u is false (candidate 0), u > u - 1 true
    (candidate 1), u > u + 1 false (candidate 0).  One run per j, two steps each (the second on whatever the node now holds)."""
    n, K = 64, 3 * 64
    u_a, u_n = sr.draws(SEED, LANE0, n, 1)
    u = u_a if which == "action" else u_n
    assert ((u > 0) & (u < 0xFFFFFFFF)).all()                           # nothing wraps
    thr = (u[:, None] + np.array([0, -1, 1]).astype(np.uint32)[None, :]).astype(np.uint32).reshape(K)
    succ = (np.arange(K) + 3) % K                                        # candidate 1 of `next`: the same j of the next lane
    if which == "action":
        action, athr = np.tile([LISTEN, OPEN0], (K, 1)), thr[:, None]
        nxt, nthr = np.repeat(np.arange(K)[:, None, None], 3, axis=1), np.zeros((K, 3, 0), np.uint32)
    else:
        action, athr = np.full((K, 1), LISTEN), np.zeros((K, 0), np.uint32)
        nxt = np.stack([np.repeat(np.arange(K)[:, None], 3, axis=1), np.repeat(succ[:, None], 3, axis=1)], axis=-1)
        nthr = np.repeat(thr[:, None, None], 3, axis=1)
    for j in range(3):
        start = 3 * np.arange(n) + j
        r = Run(oracle_lib, "tiger", raw(action, athr, nxt, nthr, start), n=n)
        packed, bad, _, _, node = r.reference(1)[0][:5]
        drawn = 1 if j == 1 else 0
        if which == "action":
            assert ((packed[0] & 0xFF) == (LISTEN, OPEN0)[drawn]).all(), j
        else:
            assert bad == 0 and np.array_equal(node, succ[start] if drawn else start), j
        r.check(2, r.reference(2))


def test_thresholds_in_any_order_and_at_both_ends(oracle_lib):
    """B = 4, D = 3, rows of thresholds that are not monotone, all 0 (passed by every word but 0) and all 0xFFFFFFFF (never
    passed): the pick is the count, whatever the order.  Every index the rows can give is drawn."""
    o = oracle_lib.OracleEnv("tiger")
    F, H = 0xFFFFFFFF, 0x80000000
    a_rows = np.array([[F, 0, H], [0, 0, 0], [F, F, F], [H, H >> 1, H + (H >> 1)], [H, F, 0], [0, H, 0]], np.uint32)
    n_rows = np.array([[F, 0], [0, 0], [F, F], [H, H >> 1], [0, F], [H, H]], np.uint32)
    K = len(a_rows)
    rng = np.random.RandomState(3)
    action = np.tile([LISTEN, LISTEN, LISTEN, OPEN0], (K, 1))
    nxt = rng.randint(0, K, (K, o.n_obs, 3))
    nthr = n_rows[rng.randint(0, K, (K, o.n_obs))]
    r = Run(oracle_lib, "tiger", raw(action, a_rows, nxt, nthr, rng.randint(0, K, N)))
    ref = r.reference(8, calls=2)
    u_a, _ = sr.draws(SEED, LANE0, N, 1)
    idx = sr.pick(u_a, a_rows[r.start])
    assert set(idx[r.start == 0]) == {1, 2} and set(idx[r.start == 1]) == {3} and set(idx[r.start == 2]) == {0}
    assert set(idx[r.start == 3]) == {0, 1, 2, 3}
    r.check(8, ref)


# ---- 5. the smallest and the largest shapes --------------------------------------------------------------------------------------
def test_fewer_lanes_than_a_wave(oracle_lib):
    tables, start = random_tables(oracle_lib.OracleEnv("rock"), n=5)
    r = Run(oracle_lib, "rock", stoch(tables, start), n=5)
    r.check(8, r.reference(8, calls=2))


def test_a_controller_of_one_node(oracle_lib):
    o = oracle_lib.OracleEnv("tiger")
    tables, _ = random_tables(o, K=1, B=3, D=2)
    r = Run(oracle_lib, "tiger", stoch(tables, 0))
    r.check(6, r.reference(6, calls=2))


def test_every_action_a_candidate_on_battleship(oracle_lib):
    """BattleShip 5 x 5: B = n_actions = 25 candidates per node (from_dense on a random psi and eta, K = 4)"""
    import gym_pomdp_amd as gpa
    o = oracle_lib.OracleEnv("battleship")
    assert o.n_actions == 25
    rng = np.random.RandomState(9)
    psi, eta = rng.uniform(0, 1, (4, 25)), rng.uniform(0, 1, (4, o.n_obs, 4))
    psi[1, :10] = 0.0                                                    # zero-probability actions: sorted last, never drawn
    start = rng.randint(0, 4, N)
    r = Run(oracle_lib, "battleship", lambda e: gpa.StochasticController.from_dense(e, psi / psi.sum(-1, keepdims=True),
                                                                                     eta / eta.sum(-1, keepdims=True), start=start))
    assert (r.ctrl.n_act_cand, r.ctrl.n_next_cand) == (25, 4)
    ref = r.reference(STEPS["battleship"])
    lane1 = r.start == 1
    assert ((ref[0][0][0] & 0xFF)[lane1] >= 10).all() and lane1.any()
    r.check(STEPS["battleship"], ref)


LARGEST = {
    # env, K, B, D, steps: the table footprint K*B + 4*K*(B-1) + 2*K*O*D + 4*K*O*(D-1) and which staged table is at its largest
    "rock_at_the_limit": ("rock", 256, 14, 5, 8),                       # 36 864 exactly, every table several groups of rows
    "tag_at_the_limit": ("tag", 384, 8, 1, 32),                          # 36 864 exactly
    "tag_most_successors": ("tag", 604, 1, 1, 32),                       # 36 844: 18 120 successors, the last group of rows
    "tiger_most_successor_thresholds": ("tiger", 2, 1, 1024, 8),         # 36 842: 6138 thresholds, the last group of rows
    "tiger_most_action_candidates": ("tiger", 1, 7368, 2, 8),            # 36 860: 7368 candidates, 7367 thresholds
}


@pytest.mark.parametrize("case", list(LARGEST))
def test_the_largest_controllers_the_limit_admits(oracle_lib, case):
    from gym_pomdp_amd.stoch_controller import footprint
    env, K, B, D, k = LARGEST[case]
    o = oracle_lib.OracleEnv(env)
    assert 36864 - 32 < footprint(K, o.n_obs, B, D) <= 36864
    (action, ap, nxt, nxp), start = random_tables(o, K=K, B=B, D=D, seed=11)
    if env == "tag":
        action[:] = action % 4                                           # moves only: nobody tags, no episode ends early
    start[0], nxt[K - 1] = K - 1, K - 1                                  # lane 0 stands on the last node throughout: the tables' ends
    ap[:, -1] += ap.sum(-1)                                              # half of the draws take the LAST candidate: the rows' ends
    nxp[:, :, -1] += nxp.sum(-1)
    r = Run(oracle_lib, env, stoch((action, ap / ap.sum(-1, keepdims=True), nxt, nxp / nxp.sum(-1, keepdims=True)), start))
    ref = r.reference(k)
    node = ref[0][4]
    u_a, _ = sr.draws(SEED, LANE0, N, 1)
    assert sr.pick(u_a, r.tables[1][r.start]).max() == B - 1             # the last candidate of a row is drawn
    assert node[0] == K - 1
    r.check(k, ref, layouts=("packed", "returns"))


# ---- 6. refused entries --------------------------------------------------------------------------------------------------------
def test_refused_entries_leave_their_lanes_alone_and_are_counted(oracle_lib):
    """validate=False: node 5 holds an out-of-range action as candidate 1 and one that fits no byte as candidate 2, every
    candidate successor of node 6 but the first is K or -1, and lane 2 comes in on node K (lane 3 on node -1).  Lanes are left
    as the header says; the count equals the restatement's."""
    o = oracle_lib.OracleEnv("rock")
    K, k = 7, 8
    (action, ap, nxt, nxp), start = random_tables(o, K=K, B=3, D=3)
    action[5, 1], action[5, 2] = o.n_actions, 1 << 20
    action[6] = 5                                                        # check rock 0: a step that stands, a lane that lives
    nxt[6, :, 1], nxt[6, :, 2] = K, -1
    nxt[nxt == 5], nxt[nxt == 6] = 0, 1                                  # only the lanes that start there meet nodes 5 and 6
    nxt[5], nxt[6, :, 0] = 5, 6
    start[:4] = [5, 6, K, -1]
    start[4:][start[4:] >= 5] = 0
    import gym_pomdp_amd as gpa
    r = Run(oracle_lib, "rock", lambda e: gpa.StochasticController(e, action, ap, nxt, nxp, start=start, validate=False))
    ref = r.reference(k)
    packed, bad, st, done, node = ref[0][:5]
    b0 = packed[:, 0] & 0xFF
    assert set(b0) >= {o.n_actions, 255}                                 # both refused candidates are drawn
    assert (packed[:, 1] & 0xFF == 5).all() and not (packed[:, 1] >> 24).any()          # lane 1 steps, and stays on node 6
    assert (packed[:, 2] == 255).all() and (packed[:, 3] == 255).all()
    assert np.array_equal(st[:, 2:4], r.st0[:, 2:4]) and node[:4].tolist() == [5, 6, K, -1] and not done[1:4].any()
    assert 2 * k + int((b0 >= o.n_actions).sum()) < bad <= 3 * k + int((b0 >= o.n_actions).sum())
    r.check(k, ref)


def test_an_observation_without_a_column_finds_no_successor(oracle_lib):
    """Tag built with obs_cells = 20: the env observes 21 values, the agent's cells 21 .. 28 have no column — the step stands,
    the node stays, counted"""
    o = oracle_lib.OracleEnv("tag", obs_cells=20)
    assert o.n_obs == 21
    tables, start = random_tables(o)
    tables[0][:] = tables[0] % 4
    r = Run(oracle_lib, "tag", stoch(tables, start), obs_cells=20)
    ref = r.reference(16)
    assert ref[0][1] > 0 and ((ref[0][0] >> 8 & 0xFF) > 20).any()
    r.check(16, ref)


# ---- 7. frozen lanes -----------------------------------------------------------------------------------------------------------
def test_lanes_frozen_on_entry_keep_drawing_their_action_byte(oracle_lib):
    """every third lane and a whole wave (lanes 256 .. 319) are done on entry: their records carry the drawn action byte | 1 <<
    24 — it changes from step to step — and their node and state are untouched"""
    tables, start = random_tables(oracle_lib.OracleEnv("rock"))
    r = Run(oracle_lib, "rock", stoch(tables, start))
    done0 = (np.arange(N) % 3 == 0).astype(np.uint8)
    done0[256:320] = 1
    ref = r.reference(8, done0=done0)
    packed, bad, st, done, node = ref[0][:5]
    fz = done0 != 0
    assert (packed[:, fz] >> 8 == 1 << 16).all() and (packed[:, fz] & 0xFF).std(axis=0).max() > 0
    assert np.array_equal(st[:, fz], r.st0[:, fz]) and np.array_equal(node[fz], r.start[fz]) and done[fz].all()
    r.check(8, ref, done0=done0)


# ---- 8. sharding ---------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_one_batch(oracle_lib):
    """two envs of 512 lanes at lane_offset 0 and 512 equal one env of 1024 lanes: every draw is a function of the global lane"""
    import gym_pomdp_amd as gpa
    k = 16
    o = oracle_lib.OracleEnv("tag")
    tables, start = random_tables(o, n=1024)

    def play(n, lane0, st):
        e = gpa.make(ENV_IDS["tag"], batch_size=n, seed=SEED, lane_offset=lane0, auto_reset=False)
        e.reset()
        c = gpa.StochasticController(e, *tables, start=st)
        rows = rows_of(e.run_controller(c, k, layout="packed"), k, n)
        return rows, np_(e.state), np_(e._done), np_(c.node)
    whole = play(1024, 0, start)
    lo, hi = play(512, 0, start[:512]), play(512, 512, start[512:])
    for w, a, b in zip(whole, lo, hi):
        assert np.array_equal(w, np.concatenate([a, b], axis=-1))


# ---- 9. frequencies ------------------------------------------------------------------------------------------------------------
def test_each_action_is_drawn_as_often_as_psi_says(oracle_lib):
    """the host test's case and seed (Tiger, one node, psi = (.5, .3, .2), 65 536 lanes, one step) on the device: the counts are
    the restatement's, hence within 5 sigma of n p"""
    import gym_pomdp_amd as gpa
    want, packed, st, done = frequency_case(oracle_lib)
    e = gpa.make(ENV_IDS["tiger"], batch_size=FREQ_N, seed=FREQ_SEED, auto_reset=False)
    e.reset()
    c = gpa.StochasticController(e, [[0, 1, 2]], [list(FREQ_P)], np.zeros((1, 3, 1), int), np.ones((1, 3, 1)))
    rows = rows_of(e.run_controller(c, 1, layout="packed"), 1, FREQ_N)
    got = np.bincount(rows[0] & 0xFF, minlength=3)
    print("counts", got.tolist())
    assert np.array_equal(got, want) and within_five_sigma(got)
    assert np.array_equal(rows, packed) and np.array_equal(np_(e.state).view(np.uint32), st) and np.array_equal(np_(e._done), done)


# ---- 10. the episode loop end to end ---------------------------------------------------------------------------------------------
def test_finished_lanes_restart_on_their_start_node(oracle_lib):
    """Tiger under an epsilon-soft "listen twice, open the other door": run, ctrl.reset_nodes(where=env.done),
    env.reset(where=env.done), run again — the second run equals the restatement from the masked reset's state with the
    finished lanes back on node 0"""
    import gym_pomdp_amd as gpa
    OPEN1 = 1
    action = [LISTEN, LISTEN, LISTEN, OPEN1, OPEN0]
    nxt = [[1, 2, 0], [3, 0, 0], [0, 4, 0], [0, 0, 0], [0, 0, 0]]
    k = 16
    r = Run(oracle_lib, "tiger", lambda e: gpa.StochasticController.epsilon_soft(gpa.Controller(e, action, nxt), .2))
    _, _, st, done, node = r.reference(k)[0][:5]
    fin = done.astype(bool)
    assert fin.any() and not fin.all()
    r.rewind()
    r.e.run_controller(r.ctrl, k)
    r.ctrl.reset_nodes(where=r.e.done)
    t = r.e.call_counter
    ob = r.e.reset(where=r.e.done)
    fresh = r.o.new_state(N)
    want_ob = r.o.batch_reset(fresh, SEED, LANE0, t, nthreads=r.nt)
    assert np.array_equal(np_(ob), np.where(fin, want_ob, -1)) and not bool(r.e.done.any())
    st, node, done = np.where(fin[None, :], fresh, st).astype(np.uint32), np.where(fin, 0, node), np.zeros(N, np.uint8)
    assert np.array_equal(np_(r.ctrl.node), node)
    packed, bad = sr.run(r.o, st, done, node, *r.tables, k, SEED, LANE0, t + 1, nthreads=r.nt)
    out = r.e.run_controller(r.ctrl, k, layout="packed")
    assert np.array_equal(rows_of(out, k, N), packed) and bad == 0 == r.e.invalid_action_count()
    assert np.array_equal(np_(r.e.state).view(np.uint32), st) and np.array_equal(np_(r.ctrl.node), node)
    assert np.array_equal(np_(r.e._done), done)
