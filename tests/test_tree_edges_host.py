"""The four tree searches at the edges of the Philox key and counter and under every env form, without a GPU: the coordinate
sets, the case tables and the oracle-side roots that tests/test_gpu_tree_edges.py runs on the device, the coverage each shape
must reach (asserted here on the restatements alone, before anything runs on a GPU), and the proof that the edges matter: at
every coordinate set a restatement with one coordinate damaged — the key's high word dropped, the counter kept in 32 bits,
the lanes taken mod 2^31, the ROLLOUT counter taken at t_s instead of t_s + k0 — returns other simulations, so the device
comparison of the same case fails under the corresponding kernel bug.

    K1  seed 0x9E3779B97F4A7C15; lane_offset = 2^32 / W - R, so the last tree is global lane 2^32 - 1 and the idle threads of
        its workgroup wrap past 0; the call counter carries into its high word at step 1 of simulation S / 2, so every lane
        that leaves the tree in that simulation has t_s < 2^32 <= t_s + k0.  For the kept trees the first search ends at
        2^32 - 1: the first real step's own counter is the first with t_hi = 1 and every later search runs above the carry
    K2  seed 2^32 (k0 = 0, k1 = 1), lane0 = 2^22, counter 0xFFFFFFFE_FFFFFFF9: t_hi turns 0xFFFFFFFF seven steps in
    K3  seed 2^64 - 1, lane 0, counter 0"""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import particle_restatement as pr  # noqa: E402
import preferred_rollout_restatement as rr  # noqa: E402
import tree_keep_preferred_restatement as kp  # noqa: E402
import tree_keep_restatement as tk  # noqa: E402
import tree_search_preferred_restatement as tp  # noqa: E402
import tree_search_restatement as ts  # noqa: E402
from oracle import oracle_lib as ol  # noqa: E402

M32, M64 = 0xFFFFFFFF, ts.M64
KS = ("K1", "K2", "K3")
SEEDS = {"K1": 0x9E3779B97F4A7C15, "K2": 1 << 32, "K3": (1 << 64) - 1}
WARM, WARM_SEED = 2, 4242                     # test_gpu_tree_search.setup: two steps under RandomState(4242)'s actions
PREP, ROOT_SEED = 6, 1                        # test_gpu_tree_search_preferred.py's roots
TEN = ("tree_visits", "tree_q", "n_nodes", "sim_ret", "sim_steps", "sim_tree_steps", "q", "visits", "best", "value")
UCB = {"tiger": 10.0, "tag": 10.0, "network": 10.0, "rock": 20.0, "stochrock": 20.0, "battleship": 5.0}
PRIORS = [(0, 0.0), (3, 5.0), (1, -20.0)]        # the last for the kept trees: under (3, 5.0) RockSample's best action at S = 9 is one
PRIOR_NAMES = ["no-priors", "n3-v5", "n1-v-20"]  # that only its priors visited, and no tree holds its child
ROCK15 = dict(board_size=15, num_rocks=15)


def discount_of(env):
    return 1.0 if env == "battleship" else .95


def kwid(env, kw):
    return env + "".join("-%s" % ("x".join(str(x) for x in v) if isinstance(v, tuple) else v) for v in kw.values())


# ---- coordinates ------------------------------------------------------------------------------------------------------------
def coords(K, R, W, S, D, resume=False):
    """(seed, lane_offset, t0): the trees' lanes are (lane_offset + r) * W + w, t0 the call counter of the (first) search"""
    if K == "K1":
        assert (1 << 32) % W == 0 and S >= 2 and D >= 2
        return SEEDS[K], (1 << 32) // W - R, (1 << 32) - (S * D if resume else (S // 2) * D + 1)
    if K == "K2":
        assert (1 << 22) % W == 0
        return SEEDS[K], (1 << 22) // W, 0xFFFFFFFEFFFFFFF9
    return SEEDS[K], 0, 0


def carry_of(t0, S, D):
    """the first (s, k) of a search from t0 whose step counter has another high word than t0, or None"""
    for s in range(S):
        for k in range(D):
            if ((t0 + s * D + k) & M64) >> 32 != t0 >> 32:
                return s, k
    return None


def designed_carry(K, S, D, resume=False):
    if K == "K1":
        return None if resume else (S // 2, 1)
    if K == "K2":
        return (7 // D, 7 % D) if 7 < S * D else None
    return None


def edge_coverage(want, K, R, W, S, D, P, seed, lane0, t0, resume=False):
    """what a part-1 shape must reach, from the restatement's result alone -> a dict of what was seen"""
    n = R * W
    carry = carry_of(t0, S, D)
    assert carry == designed_carry(K, S, D, resume), (K, carry)
    if K == "K1":
        assert lane0 + n == 1 << 32 and lane0 % 4 == 0                       # the last tree is lane 2^32 - 1
        assert resume or carry[0] >= 1
        assert not resume or (t0 + S * D) == 1 << 32                         # the real step's own counter is the first with t_hi = 1
    steps, tsteps = want["sim_steps"], want["sim_tree_steps"]
    rolled = steps > tsteps                                                  # left the tree at k0 = tsteps and drew ROLLOUT words
    seen = dict(carry=carry, longest_rollout=int((steps - tsteps).max()), across=0)
    if carry is not None:
        s, k = carry
        # ROLLOUT at t_s + k0 on the far side of the carry from t_s: k0 >= k (k >= 1)
        seen["across"] = int((rolled[s] & (tsteps[s] >= k)).sum()) if k >= 1 else 0
        if K == "K1" or k == 1:
            assert seen["across"] >= 1, (K, seen)
    assert seen["longest_rollout"] > 4, (K, seen)                            # a second ROLLOUT block
    if P:
        cols = set()
        per_root = [set() for _ in range(R)]
        for s in range(S):
            x = ts.tree_words(seed, lane0, n, (t0 + s * D) & M64)
            c = ((x * np.uint64(P)) >> np.uint64(32)).astype(np.int64)
            for i in range(n):
                per_root[i // W].add(int(c[i]))
        seen["columns"] = min(len(c) for c in per_root)
        assert seen["columns"] >= 2, (K, seen)                               # the TREE word picks among the particles
    return seen


# ---- roots on the oracle alone ----------------------------------------------------------------------------------------------
def uniform_roots(env, kw, R, lane_offset, seed, P=0):
    """test_gpu_tree_search.setup on the oracle: reset() at call 0, two steps under RandomState(4242)'s actions, a
    ParticleBelief of the default seed that followed them -> (oracle, states, particles | None, done flags, the belief's seed)"""
    o = ol.OracleEnv(env, **kw)
    st = o.new_state(R)
    ob = o.batch_reset(st, seed, lane_offset, 0)
    bseed = (seed + rr.BELIEF_SEED_OFFSET) & M64
    parts = pr.init(o, None, R, P, bseed, lane_offset * P, 0, ob=ob)[0] if P else None
    rs = np.random.RandomState(WARM_SEED)
    done = np.zeros(R, np.uint8)
    for k in range(WARM):
        a = rs.randint(0, o.n_actions, R).astype(np.int32)
        ob, rew, done, _ = o.batch_step(st, a, seed, lane_offset, 1 + k, auto_reset=False, done=done)
        if P:
            parts, _ = pr.update(o, parts, a, ob, rew, done, False, R, P, bseed, lane_offset * P, 1 + k)
    return o, st, parts, np.asarray(done, np.uint8), bseed


def preferred_roots(env, kw, R, lane_offset, seed, P=0):
    """test_gpu_preferred.constructed on the oracle: reset(), six heuristic-policy steps, rr.construct_roots over them
    -> (oracle, state columns [words, R * max(P, 1)], belief | None, history, prev_ob, true states, done flags)"""
    o = ol.OracleEnv(env, **kw)
    got = rr.prepare_roots(o, R, PREP, seed, lane_offset, nthreads=ol.max_threads(), P=max(P, 1))
    st, belief, history, pob, done = got[:5]
    cols = got[5] if P else st
    belief, history, pob = rr.construct_roots(o, cols, max(P, 1), belief, history, pob, ROOT_SEED)
    return o, cols, belief, history, pob, st, (np.asarray(done) != 0).astype(np.uint8)


def run_uniform(env, kw, K, row, c=None, discount=None, mutate=None, seed=None, lane0=None):
    """ts.search of a (R, W, S, D, P) row at a coordinate set -> (result, (seed, lane0, t0)); seed / lane0: damaged ones"""
    R, W, S, D, P = row
    sd, lane_offset, t0 = coords(K, R, W, S, D)
    o, st, parts, _, _ = uniform_roots(env, kw, R, lane_offset, sd, P)
    sd, l0 = sd if seed is None else seed, lane_offset * W if lane0 is None else lane0
    want = ts.search(o, st, R, W, S, D, discount_of(env) if discount is None else discount, UCB[env] if c is None else c, sd, l0, t0,
                     particles=parts, P=P, nthreads=ol.max_threads(), mutate=mutate)
    return want, (sd, l0, t0), o


def run_preferred(env, kw, K, row, prior, c=None, mutate=None, seed=None, lane0=None):
    R, W, S, D, P = row
    sd, lane_offset, t0 = coords(K, R, W, S, D)
    o, cols, belief, history, pob, _, _ = preferred_roots(env, kw, R, lane_offset, sd, P)
    sd, l0 = sd if seed is None else seed, lane_offset * W if lane0 is None else lane0
    want = tp.search(o, cols, belief, history, pob, R, W, S, D, discount_of(env), UCB[env] if c is None else c, sd, l0, t0, P=P,
                     prior_n=prior[0], prior_v=prior[1], nthreads=ol.max_threads(), mutate=mutate)
    return want, (sd, l0, t0), o


def play_uniform(env, kw, seed, lane_offset, t0, row, Cn, steps, c=None, discount=None):
    """search_step(tree=) over `steps` real steps on the oracle alone -> (the searches' results, the largest kept tree after
    each advance)"""
    R, W, S, D, P = row
    o, st, parts, frozen, bseed = uniform_roots(env, kw, R, lane_offset, seed, P)
    gamma, c = discount_of(env) if discount is None else discount, UCB[env] if c is None else c
    logn, trees, t, tb, res, kept = ts.log_table(steps * S), None, t0, 1 + WARM, [], []
    for _ in range(steps):
        want = tk.search(o, st, R, W, S, D, gamma, c, seed, lane_offset * W, t, trees=trees, C=Cn, logn=logn, particles=parts, P=P,
                         nthreads=ol.max_threads())
        res.append(want)
        t += S * D
        real = st.copy()
        ob, rew, done, _ = o.batch_step(real, want["best"], seed, lane_offset, t, auto_reset=False, done=frozen.copy())
        t += 1
        if P:
            parts, _ = pr.update(o, parts, want["best"], ob, rew, done, False, R, P, bseed, lane_offset * P, tb)
            tb += 1
        trees = tk.advance(want["trees"], W, want["best"], ob.astype(np.int32), (done != 0).astype(np.uint8))
        kept.append(int(tk.n_nodes_of(trees).max()))
        st, frozen = real, (done != 0).astype(np.uint8) | frozen
    return res, kept


def play_preferred(env, kw, seed, lane_offset, t0, row, Cn, steps, prior, c=None):
    """search_step(policy="preferred", history=, tree=[, belief=]) over `steps` real steps on the oracle alone
    -> (the searches' results, the largest kept tree after each advance)"""
    R, W, S, D, P = row
    o, cols, belief, history, pob, st, frozen = preferred_roots(env, kw, R, lane_offset, seed, P)
    c = UCB[env] if c is None else c
    bseed, tb = (seed + rr.BELIEF_SEED_OFFSET) & M64, 1 + PREP
    logn, trees, t, res, kept = kp.log_table(steps, S, o.n_actions, prior[0]), None, t0, [], []
    for _ in range(steps):
        want = kp.search(o, cols if P else st, belief, history, pob, R, W, S, D, discount_of(env), c, seed, lane_offset * W, t, trees=trees,
                         C=Cn, logn=logn, P=P, prior_n=prior[0], prior_v=prior[1], nthreads=ol.max_threads())
        res.append(want)
        t += S * D
        best = want["best"]
        real = st.copy()
        ob, rew, done, _ = o.batch_step(real, best, seed, lane_offset, t, auto_reset=False, done=frozen.copy())
        t += 1
        if P:
            cols, _ = pr.update(o, cols, best, ob, rew, done, False, R, P, bseed, lane_offset * P, tb)
            tb += 1
        bel, hs, p = rr.expand(o, belief, history, pob, R, 1)
        live = frozen == 0
        if bel is not None:
            bel.update(real, np.where(live, best, 0).astype(np.int32), np.where(live, ob, 0).astype(np.int32),
                       np.where(live, done, 1).astype(np.uint8), auto_reset=False)
            belief = {f: getattr(bel, f).copy() for f, _ in ol.Belief.FIELDS}
        hs.append(p, best.astype(np.int32), ob.astype(np.int32), done, auto_reset=False)
        history = {f: getattr(hs, f).copy() for f in history}
        pob = np.ascontiguousarray(ob.astype(np.int32))
        trees = tk.advance(want["trees"], W, best, ob.astype(np.int32), (done != 0).astype(np.uint8))
        kept.append(int(tk.n_nodes_of(trees).max()))
        st, frozen = real, (done != 0).astype(np.uint8) | frozen
    return res, kept


# ---- part 1: the cases ---------------------------------------------------------------------------------------------------------
U_ENVS = [("tiger", {}), ("rock", {}), ("rock", ROCK15), ("tag", {}), ("battleship", {}), ("network", {})]
U_NAMES = ["tiger", "rock7-8", "rock15-15", "tag", "battleship5x5", "network"]
P_ENVS = [("rock", {}), ("rock", ROCK15), ("stochrock", {}), ("tag", {})]
P_NAMES = ["rock7-8", "rock15-15", "stochrock", "tag"]
# (R, W, S, D, P)
ROW = (8, 4, 9, 6, 0)                          # enough for the carry: 32 trees, rollouts of up to five steps
ROW_P = (8, 8, 9, 10, 8)                       # the TREE word and ROLLOUT block 1 at the edge key; W = P, so that at K1 the belief's
#                                                lanes (lane_offset * P + r * P + j) end at 2^32 - 1 as the trees' do
ROW_W1 = (8, 1, 9, 6, 0)                       # W = 1: lane_offset = 2^32 - R at K1
ROW_NAMES = {ROW: "8x4-S9-D6", ROW_P: "8x8-S9-D10-P8", ROW_W1: "8x1-S9-D6"}
# uniform search: (index into U_ENVS, K, row)
U_SEARCH = [(i, "K1", ROW) for i in range(6)] + [(i, K, ROW) for K in ("K2", "K3") for i in (1, 3)] + \
           [(3, "K1", ROW_P), (1, "K2", ROW_P), (3, "K1", ROW_W1)]
# preferred search: (index into P_ENVS, K, row, index into PRIORS)
P_SEARCH = [(i, "K1", ROW, p) for i in range(4) for p in (1, 0)] + [(i, K, ROW, p) for K in ("K2", "K3") for i in (0, 3) for p in (1, 0)] + \
           [(0, "K1", ROW_P, 1), (3, "K2", ROW_P, 0)]
# kept trees, three real steps, C = 2 S + 1: (index, K, row)
U_RESUME = [(0, "K1", ROW), (3, "K1", ROW), (5, "K1", ROW), (1, "K2", ROW), (3, "K1", ROW_P)]
P_RESUME = [(i, K, ROW, 2) for K in ("K1", "K2") for i in (0, 3)] + [(0, "K1", ROW_P, 2)]
STEPS = 3


def u_id(c):
    return "%s-%s-%s" % (U_NAMES[c[0]], c[1], ROW_NAMES[c[2]])


def p_id(c):
    return "%s-%s-%s-%s" % (P_NAMES[c[0]], c[1], ROW_NAMES[c[2]], PRIOR_NAMES[c[3]])


@pytest.mark.parametrize("case", U_SEARCH, ids=[u_id(c) for c in U_SEARCH])
def test_the_uniform_rows_reach_the_edges(case):
    ei, K, row = case
    want, (seed, lane0, t0), _ = run_uniform(U_ENVS[ei][0], U_ENVS[ei][1], K, row)
    R, W, S, D, P = row
    print(u_id(case), edge_coverage(want, K, R, W, S, D, P, seed, lane0, t0))


@pytest.mark.parametrize("case", P_SEARCH, ids=[p_id(c) for c in P_SEARCH])
def test_the_preferred_rows_reach_the_edges(case):
    ei, K, row, pi = case
    want, (seed, lane0, t0), _ = run_preferred(P_ENVS[ei][0], P_ENVS[ei][1], K, row, PRIORS[pi])
    R, W, S, D, P = row
    print(p_id(case), edge_coverage(want, K, R, W, S, D, P, seed, lane0, t0))
    assert want["stats"]["nan_prob"] == 0


def resume_coverage(res, kept, K, row, seed, lane0, t0):
    """a resume row: the first search's edges, and a tree kept over the first real step (at K1 the step whose counter is the
    first with t_hi = 1, so the kept tree is resumed on the far side of the carry)"""
    R, W, S, D, P = row
    seen = edge_coverage(res[0], K, R, W, S, D, P, seed, lane0, t0, resume=True)
    assert kept[0] >= 1 and (res[1]["n_nodes"] > 1).any(), kept
    return dict(seen, kept=kept)


@pytest.mark.parametrize("case", U_RESUME, ids=[u_id(c) for c in U_RESUME])
def test_the_uniform_resume_rows_keep_a_tree_across_the_carry(case):
    ei, K, row = case
    R, W, S, D, P = row
    seed, lane_offset, t0 = coords(K, R, W, S, D, resume=True)
    res, kept = play_uniform(U_ENVS[ei][0], U_ENVS[ei][1], seed, lane_offset, t0, row, 2 * S + 1, STEPS)
    print(u_id(case), resume_coverage(res, kept, K, row, seed, lane_offset * W, t0))


@pytest.mark.parametrize("case", P_RESUME, ids=[p_id(c) for c in P_RESUME])
def test_the_preferred_resume_rows_keep_a_tree_across_the_carry(case):
    ei, K, row, pi = case
    R, W, S, D, P = row
    seed, lane_offset, t0 = coords(K, R, W, S, D, resume=True)
    res, kept = play_preferred(P_ENVS[ei][0], P_ENVS[ei][1], seed, lane_offset, t0, row, 2 * S + 1, STEPS, PRIORS[pi])
    print(p_id(case), resume_coverage(res, kept, K, row, seed, lane_offset * W, t0))


# ---- part 2: the edges matter ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def counters_in_32_bits(o):
    """every counter the restatements hand on — the env's step, the TREE word, the ROLLOUT stream — cut to its low word: a
    kernel that lost the carry into t_hi (or ignored t_hi)"""
    step, words_ts, words_tp, tree = o.batch_step, ts.stream_words, tp.stream_words, ts.tree_words
    o.batch_step = lambda st, a, seed, lane0, t, **kw: step(st, a, seed, lane0, t & M32, **kw)
    ts.stream_words = lambda seed, lane, t, stream, n: words_ts(seed, lane, t & M32, stream, n)
    tp.stream_words = lambda seed, lane, t, stream, n: words_tp(seed, lane, t & M32, stream, n)
    ts.tree_words = lambda seed, lane0, n, t: tree(seed, lane0, n, t & M32)
    try:
        yield
    finally:
        del o.batch_step
        ts.stream_words, tp.stream_words, ts.tree_words = words_ts, words_tp, tree


# which damage changes the coordinates of which set: the others leave every word of every key and counter as it was, and the
# test asserts THAT (the same simulations) instead of skipping
APPLIES = {"K1": {"seed", "counter", "lanes", "k0"}, "K2": {"seed", "counter", "k0"}, "K3": {"seed", "k0"}}
DAMAGE_ROW = (8, 8, 9, 10, 8)                  # ROW_P: with particles, so that the TREE word is among the damaged draws


@pytest.mark.parametrize("search", ["uniform", "preferred"])
@pytest.mark.parametrize("K", KS)
def test_a_damaged_coordinate_changes_the_simulations(K, search):
    """tag under the uniform and under the preferred restatement (priors (3, 5.0)), 64 trees from 8 particles: the real
    coordinates against each damage.  sim_ret differs for every damage that changes a word at this coordinate set and is
    the same, bit for bit, for the others — K2's and K3's lanes are below 2^31, K3's counters below 2^32."""
    run = (lambda **kw: run_uniform("tag", {}, K, DAMAGE_ROW, **kw)) if search == "uniform" else \
          (lambda **kw: run_preferred("tag", {}, K, DAMAGE_ROW, PRIORS[1], **kw))
    real, (seed, lane0, t0), o = run()
    R, W, S, D, P = DAMAGE_ROW
    assert int((real["sim_steps"] - real["sim_tree_steps"]).max()) > 4
    damaged = {"seed": run(seed=seed & M32)[0], "lanes": run(lane0=lane0 % (1 << 31))[0], "k0": run(mutate="k0_at_root")[0]}
    R, W, S, D, P = DAMAGE_ROW
    sd, lane_offset, _ = coords(K, R, W, S, D)
    if search == "uniform":
        o, st, parts, _, _ = uniform_roots("tag", {}, R, lane_offset, sd, P)
        with counters_in_32_bits(o):
            damaged["counter"] = ts.search(o, st, R, W, S, D, .95, UCB["tag"], seed, lane0, t0, particles=parts, P=P)
    else:
        o, cols, belief, history, pob, _, _ = preferred_roots("tag", {}, R, lane_offset, sd, P)
        with counters_in_32_bits(o):
            damaged["counter"] = tp.search(o, cols, belief, history, pob, R, W, S, D, .95, UCB["tag"], seed, lane0, t0, P=P, prior_n=3,
                                           prior_v=5.0)
    assert (seed & M32 != seed) == ("seed" in APPLIES[K]) and (lane0 % (1 << 31) != lane0) == ("lanes" in APPLIES[K])
    assert ((t0 + S * D - 1) >> 32 != 0) == ("counter" in APPLIES[K])
    for what, got in damaged.items():
        differs = got["sim_ret"].tobytes() != real["sim_ret"].tobytes()
        assert differs == (what in APPLIES[K]), (K, search, what)
        if what not in APPLIES[K]:                                          # nothing changed: every output is the same
            assert all(got[k].tobytes() == real[k].tobytes() for k in TEN), (K, search, what)


# ---- part 3: env configurations ---------------------------------------------------------------------------------------------
CFG_SEED, CFG_LANE0, CFG_T0 = 0x9E3779B97F4A7C15, 1 << 22, (1 << 33) + 5   # tests/test_env_params_host.py's coordinates
ROW_A = (6, 4, 33, 10, 0)
ROW_B = (70, 4, 2, 2, 4)
ROW_A8 = (12, 4, 9, 10, 8)                     # the preferred search's particle row
RING, LEGS = 2, 3
U_CONFIGS = [("stochrock", {}), ("stochrock", dict(p_move=.4)), ("stochrock", dict(p_move=.95)), ("stochrock", dict(p_move=.5)),
             ("stochrock", dict(board_size=15, num_rocks=15, p_move=.4)),
             ("rock", dict(board_size=11, num_rocks=11)), ("rock", dict(board_size=4, num_rocks=3)), ("rock", dict(board_size=2, num_rocks=1)),
             ("tag", dict(move_prob=.3)), ("tag", dict(move_prob=.55)), ("tag", dict(move_prob=.5)),
             ("tag", dict(num_opponents=2, move_prob=.3)), ("tag", dict(num_opponents=4, move_prob=.4)),
             ("tag", dict(obs_cells=63)), ("tag", dict(obs_cells=64))] + \
            [("network", dict(n_machines=M, problem_type=T)) for M, T in ((1, RING), (4, LEGS), (17, RING), (25, LEGS), (32, RING), (16, RING))] + \
            [("battleship", dict(board_size=(8, 6), max_len=4)), ("battleship", dict(board_size=(10, 10), max_len=5))]
P_CONFIGS = [("rock", dict(board_size=11, num_rocks=11)), ("rock", dict(board_size=4, num_rocks=3)),
             ("stochrock", dict(p_move=.4)), ("stochrock", dict(p_move=.95)), ("stochrock", dict(board_size=15, num_rocks=15, p_move=.4)),
             ("tag", dict(move_prob=.3)), ("tag", dict(num_opponents=2, move_prob=.3)), ("tag", dict(num_opponents=4, move_prob=.4)),
             ("tag", dict(obs_cells=64))]
NET32 = ("network", dict(n_machines=32, problem_type=RING))
SHIP10 = ("battleship", dict(board_size=(10, 10), max_len=5))
# the wide envs: (env, kw, (R, W, S, D, P), ucb_c), greedy so that the root's best action is taken again and again and its
# child runs out of untried actions.  Network-32 (A = 65): S = 212 — at 2 A + 8 = 138 and at 203 the restatement reaches two
# tree steps but no second child on any edge below the root.  BattleShip 10x10 (A = 100): S = 2 A + 8 = 208, from 4 particles:
# a shot's outcome is a function of the state, so from the true states an edge never gets a second child.
WIDE = [NET32 + ((3, 4, 212, 6, 0), 0.0), SHIP10 + ((3, 4, 2 * 100 + 8, 6, 4), 0.0)]
U_KEEP = [("stochrock", dict(p_move=.4)), ("tag", dict(num_opponents=2)), NET32, SHIP10]
P_KEEP = [("stochrock", dict(p_move=.4)), ("tag", dict(num_opponents=2))]
KEEP_ROW = (6, 4, 9, 6, 0)
ROCK_BRANCHES = ("fallback", "sample_rule", "check_ok_cleared", "move_bit_up", "move_bit_down", "sample_bit_up", "sample_bit_down")


def cfg_uniform(env, kw, row, c=None, discount=None):
    """a part-3 row of the uniform search on the oracle -> (oracle, states, particles, result)"""
    R, W, S, D, P = row
    o, st, parts, _, _ = uniform_roots(env, kw, R, CFG_LANE0 // W, CFG_SEED, P)
    want = ts.search(o, st, R, W, S, D, discount_of(env) if discount is None else discount, UCB[env] if c is None else c, CFG_SEED,
                     CFG_LANE0, CFG_T0, particles=parts, P=P, nthreads=ol.max_threads())
    return o, st, parts, want


def cfg_preferred(env, kw, row, prior):
    R, W, S, D, P = row
    o, cols, belief, history, pob, _, _ = preferred_roots(env, kw, R, CFG_LANE0 // W, CFG_SEED, P)
    return tp.search(o, cols, belief, history, pob, R, W, S, D, discount_of(env), UCB[env], CFG_SEED, CFG_LANE0, CFG_T0, P=P,
                     prior_n=prior[0], prior_v=prior[1], nthreads=ol.max_threads())


def wide_coverage(o, st, parts, want, row, c, discount):
    """the tree structure of a wide row, from the kept-tree restatement of the same search (C = S + 1 from empty trees: its ten
    keys are ts.search's, asserted): some tree is two steps deep, and some node other than the root has two children on one
    edge — a sibling chain below the root, at a row pitch of A edges"""
    R, W, S, D, P = row
    k = tk.search(o, st, R, W, S, D, discount, c, CFG_SEED, CFG_LANE0, CFG_T0, particles=parts, P=P, nthreads=ol.max_threads())
    assert all(k[key].tobytes() == want[key].tobytes() for key in TEN)
    deepest = int(want["sim_tree_steps"].max())
    chains = 0
    for t in k["trees"]:
        for h in range(1, len(t.N)):
            acts = [a for a, _ in t.children[h]]
            chains += len(acts) - len(set(acts))
    assert deepest >= 2 and chains >= 1, (deepest, chains)
    return dict(deepest=deepest, chains=chains, nodes=int(want["n_nodes"].max()))


WIDE_IDS = ["network32-S212", "battleship10x10-S208-P4"]


@pytest.mark.parametrize("env,kw,row,c", WIDE, ids=WIDE_IDS)
def test_the_wide_rows_grow_below_the_root(env, kw, row, c):
    o, st, parts, want = cfg_uniform(env, kw, row, c)
    assert o.n_actions > 64
    print(env, wide_coverage(o, st, parts, want, row, c, discount_of(env)))


def branch_totals(results):
    """[(env, kw, stats)] of preferred searches -> Tag's two counters per configuration over its rows, RockSample's over the
    union of its configurations (stochrock (15,15) alone reaches no fallback at six roots); asserted"""
    rock, tag = {c: 0 for c in ROCK_BRANCHES}, {}
    for env, kw, stats in results:
        assert stats["nan_prob"] == 0, (env, kw)
        if env == "tag":
            t = tag.setdefault(kwid(env, kw), dict(corner_tag=0, empty_history_all_five=0))
            for c in t:
                t[c] += stats[c]
        else:
            for c in rock:
                rock[c] += stats[c]
    assert all(v >= 1 for v in rock.values()), rock
    assert all(v >= 1 for t in tag.values() for v in t.values()), tag
    return rock, tag


def test_the_preferred_configurations_reach_the_policys_branches():
    """Row A and the particle row under priors (3, 5.0), a subset of what the device test runs and adds up"""
    res = [(env, kw, cfg_preferred(env, kw, row, PRIORS[1])["stats"]) for env, kw in P_CONFIGS for row in (ROW_A, ROW_A8)]
    assert len({kwid(e, k) for e, k, _ in res if e == "tag"}) == 4
    print(branch_totals(res))


def test_the_configurations_keep_subtrees():
    """three real steps with C = 2 S + 1 on the part-3 resume configurations: some tree keeps two nodes or more"""
    R, W, S, D, P = KEEP_ROW
    best = 0
    for env, kw in U_KEEP:
        _, kept = play_uniform(env, kw, CFG_SEED, CFG_LANE0 // W, CFG_T0, KEEP_ROW, 2 * S + 1, STEPS)
        best = max(best, max(kept))
    for env, kw in P_KEEP:
        _, kept = play_preferred(env, kw, CFG_SEED, CFG_LANE0 // W, CFG_T0, KEEP_ROW, 2 * S + 1, STEPS, PRIORS[2])
        best = max(best, max(kept))
    assert best >= 2, best
