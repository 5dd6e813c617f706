"""POMCP's tree search without a GPU: the C ABI's declarations and argument checks, the workspace size, the kernels'
resources, and the contract's CPU restatement (tests/tree_search_restatement.py) checked against what a search must satisfy,
on the oracle alone — with the proof that each of its rules is pinned by one of those properties."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_search_restatement as ts  # noqa: E402

NAMES = ("pomdp_tree_search_workspace", "pomdp_tree_search")


def test_entry_points_are_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    for sym in NAMES:
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in _native.SYMBOLS
        assert hasattr(_native.lib(), sym)
    assert "tree_search.hip" in _native.UNITS and "tree_pool.hip.h" in _native.HEADERS
    assert _native.ABI_VERSION == 15 and _native.lib().pomdp_abi_version() == 15
    assert re.search(r"POMDP_STREAM_TREE\s*=\s*9\b", hdr) and ts.STREAM_TREE == 9
    # the binding mirrors the header's struct field for field
    body = re.search(r"typedef struct pomdp_tree_args \{(.*?)\} pomdp_tree_args;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _native.PlanTreeArgs._fields_]
    assert C.sizeof(_native.PlanTreeArgs) == 200
    from gym_pomdp_amd.envs.base import BatchedEnv
    assert callable(BatchedEnv.search) and callable(BatchedEnv.search_step)


def _rock_params(num_rocks=8):
    from gym_pomdp_amd import _native
    p = _native.RockParams(size=7, num_rocks=num_rocks, start_x=0, start_y=3)
    for i in range(256):
        p.grid[i] = -1
    for i in range(32):
        p.thr[i] = 1 << 52
    return p


def test_bad_arguments_are_refused_before_any_launch():
    """Every check runs on the host: none of these calls reaches the GPU (fake device pointers are never dereferenced)."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    rock = _rock_params()
    A_, B_, X = 1 << 40, 1 << 41, 1 << 42           # fake "device" addresses, 16-byte aligned
    R, W, S, D = 8, 4, 16, 8
    need = L.pomdp_tree_search_workspace(0, C.byref(rock), R * W, S, D)
    assert need > 0

    def call(t0=0, **kw):
        params = kw.pop("params", rock)
        out = dict(q=X, visits=X, best=X, value=None, stride=13, reserved=0)
        out.update(kw.pop("out", {}))
        f = dict(env=0, depth=D, params=None if params is None else C.addressof(params), root_state=A_, particles=None, n_roots=R,
                 n_particles=0, trees_per_root=W, sims_per_tree=S, discount=.95, ucb_c=1.0, logn=X, workspace=B_,
                 workspace_bytes=need, tree_visits=X, tree_q=X, n_nodes=X, sim_ret=None, sim_steps=None, sim_tree_steps=None,
                 out=_native.PlanOut(**out), seed=7, lane0=0, reserved=0)
        f.update(kw)
        return L.pomdp_tree_search(C.byref(_native.PlanTreeArgs(**f)), t0, None)

    BAD = -1
    assert L.pomdp_tree_search(None, 0, None) == BAD
    assert call(params=None) == BAD
    for k in ("root_state", "logn", "workspace", "tree_visits", "tree_q", "n_nodes"):
        assert call(**{k: None}) == BAD, k
    for k in ("q", "visits", "best"):
        assert call(out={k: None}) == BAD, k
    assert call(out=dict(stride=12)) == BAD                               # stride < A = 13
    assert call(workspace_bytes=need - 1) == BAD                          # workspace too small
    assert call(workspace=B_ + 8) == BAD                                  # ... or misaligned
    assert call(lane0=2) == call(lane0=6) == BAD                          # lane0 % 4
    assert call(lane0=0xFFFFFFFC, workspace_bytes=1 << 45) == BAD         # lane0 + R * W > 2^32
    assert call(n_roots=-1) == call(trees_per_root=0) == call(sims_per_tree=0) == call(depth=-1) == BAD
    for c in (-1.0, -0.0 - 1e-300, float("nan"), float("inf")):
        assert call(ucb_c=c) == BAD, c
    for P in (2, 6, 4100, 8192):
        assert call(particles=A_, n_particles=P) == BAD, P
    assert call(particles=A_, n_particles=0) == BAD
    assert call(n_particles=8) == BAD                                     # a particle count without particles
    assert call(env=9) == BAD                                             # unknown env
    bad_rock = _rock_params()
    bad_rock.size = 99
    assert call(params=bad_rock) == -2                                    # POMDP_E_BADPARAMS
    bs = _native.BattleShipParams(x_size=16, y_size=16, max_len=5)        # 256 actions: A > 255 (or a board the layout refuses)
    assert call(env=2, params=bs, out=dict(stride=256)) in (BAD, -2)
    assert call(n_roots=0) == 0                                           # nothing to do, nothing launched
    assert call(n_roots=0, workspace=None, workspace_bytes=0) == 0


def test_workspace_size_is_monotone_in_every_argument():
    from gym_pomdp_amd import _native
    L = _native.lib()
    ws = lambda K=8, n=32, S=16, D=8: L.pomdp_tree_search_workspace(0, C.byref(_rock_params(K)), n, S, D)
    base = ws()
    assert base > 0 and base % 16 == 0
    assert ws(K=9) > base and ws(n=33) > base and ws(S=17) > base
    assert ws(D=9) > base and ws(D=16) > ws(D=15) and ws(D=17) == ws(D=16)     # the path never outgrows min(D, S) entries
    assert ws(n=64) == 2 * base
    for n in range(0, 5):
        assert ws(n=n) == n * ws(n=1)
    assert [ws(S=s) for s in range(1, 40)] == sorted(ws(S=s) for s in range(1, 40))
    assert [ws(D=d) for d in range(0, 40)] == sorted(ws(D=d) for d in range(0, 40))
    # refused shapes: 0
    assert ws(n=-1) == ws(S=0) == ws(D=-1) == ws(n=(1 << 32) + 1) == ws(S=1 << 31) == 0
    assert L.pomdp_tree_search_workspace(0, None, 32, 16, 8) == L.pomdp_tree_search_workspace(9, C.byref(_rock_params()), 32, 16, 8) == 0
    assert ws(n=1 << 32, S=1 << 20, D=64) == 0                            # more than any device holds: refused, not wrapped


def test_tree_search_kernels_keep_nothing_in_scratch_memory():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = kr.collect(units=["tree_search.hip"])
    names = [r["kernel"] for r in rows]
    assert sum(1 for k in names if k.startswith("tree_search_kernel<")) == 11          # per env type
    assert names.count("tree_merge_kernel") == 1
    bad = [(r["kernel"], r["scratch"]) for r in rows if r["scratch"] != "0"]
    assert not bad, bad


# ---- the restatement on the oracle alone ------------------------------------------------------------------------------------
SEED = 77


def _reset(o, n, seed=5):
    st = o.new_state(n)
    o.batch_reset(st, seed, 0, 0)
    return st


def prop_single_simulation_is_one_step_then_a_rollout(mutate=None):
    """W = 1, S = 1: the one simulation takes the first legal action in the tree (sim_tree_steps == 1), creates node 1 and
    rolls out: its return is r0 + discount * (the return of a _batch_rollout simulation of depth D - 1 from the state after
    that step at t0 + 1), bit for bit — the ROLLOUT words are keyed at t_s + k0, the STEP words at t_s + k.
    Mutation that fails it: `(ts + k0[i]) & M64` -> `ts` (k0_at_root)."""
    from oracle import oracle_lib as ol
    for name, kw in (("rock", {}), ("tag", {})):
        o = ol.OracleEnv(name, **kw)
        R, D, disc, lane0, t0 = 24, 9, .95, 8, 1000
        roots = _reset(o, R)
        got = ts.search(o, roots, R, 1, 1, D, disc, 1.0, SEED, lane0, t0, mutate=mutate)
        lists, lens = ol._batch_legal(o, roots)
        st = roots.copy()
        ob, rew, done, _ = o.batch_step(st, lists[:, 0].copy(), SEED, lane0, t0, auto_reset=False)
        assert not done.any()
        ro = ol._batch_rollout(o, st, 1, D - 1, disc, SEED, lane0, t0 + 1)
        want = rew.astype(np.float64) + np.float64(disc) * ro["ret"]
        assert (got["sim_tree_steps"] == 1).all() and (got["n_nodes"] == 2).all()
        assert np.array_equal(got["sim_steps"][0], 1 + ro["n_steps"])
        assert np.array_equal(got["sim_ret"][0], want), name
        assert np.array_equal(got["tree_q"][np.arange(R), lists[:, 0]], want)
        assert (got["tree_visits"].sum(axis=1) == 1).all()


def prop_unvisited_actions_are_tried_in_list_order(mutate=None):
    """Tiger, D = 1, S = 3: a fresh root tries its legal actions in list order — door 0, door 1, LISTEN — so the three
    simulations' returns are those actions' rewards in that order (the doors pay -20 / +10 by where the tiger is).
    Mutation that fails it: `fresh[0]` -> `fresh[-1]` (unvisited_last)."""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("tiger")
    R = 32
    roots = _reset(o, R)
    got = ts.search(o, roots, R, 1, 3, 1, .95, 0.0, SEED, 0, 50, mutate=mutate)
    tiger_left = (roots[0] & 1) == 0
    assert tiger_left.any() and (~tiger_left).any()
    assert np.array_equal(got["sim_ret"][0], np.where(tiger_left, -20.0, 10.0))
    assert np.array_equal(got["sim_ret"][1], np.where(tiger_left, 10.0, -20.0))
    assert (got["sim_ret"][2] == -1.0).all()
    assert (got["tree_visits"] == 1).all()


def prop_ties_go_to_the_first_maximum(mutate=None):
    """BattleShip 5 x 5, D = 1, c = 0: every shot costs 1, so after 25 simulations every V(0, a) is -1 and simulation 26 breaks
    a 25-way tie: the first entry of the legal list gets the second visit.
    Mutation that fails it: `u > bu` -> `u >= bu` (last_maximum)."""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("battleship")
    R = 4
    roots = _reset(o, R)
    lists, lens = ol._batch_legal(o, roots)
    assert (lens == 25).all()
    got = ts.search(o, roots, R, 1, 26, 1, .95, 0.0, SEED, 0, 0, mutate=mutate)
    assert (got["tree_q"] == -1.0).all()
    want = np.ones((R, 25), np.int32)
    want[np.arange(R), lists[:, 0]] = 2
    assert np.array_equal(got["tree_visits"], want)


def prop_counts_and_means_add_up(mutate=None):
    """RockSample(7,8), S = 40, D = 12: sum_a tree_visits is the number of simulations that took a step; n_nodes <= S + 1 and
    grows by at most one per simulation; sim_tree_steps <= sim_steps <= D; and the root's running means are means of sim_ret —
    sum_a N(0,a) V(0,a) equals the sum of the simulations' returns to rounding (1e-9 relative: some 40 additions of O(10)
    numbers in another order), which only holds when the backup walks from the deepest entry to the root, so that the root
    is updated with the simulation's full return.
    Mutation that fails it: `reversed(path)` -> `path` (backup_from_root)."""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("rock")
    R, W, S, D = 6, 2, 40, 12
    roots = _reset(o, R)
    got = ts.search(o, roots, R, W, S, D, .95, 5.0, SEED, 4, 7, mutate=mutate)
    assert np.array_equal(got["tree_visits"].sum(axis=1), (got["sim_steps"] > 0).sum(axis=0))
    assert (got["n_nodes"] <= S + 1).all() and (got["n_nodes"] >= 2).all()
    assert (got["sim_tree_steps"] <= got["sim_steps"]).all() and (got["sim_steps"] <= D).all()
    assert (got["sim_tree_steps"].max(axis=0) >= 2).all()                 # the trees did grow below the root
    lhs = (got["tree_visits"] * got["tree_q"]).sum(axis=1)
    rhs = got["sim_ret"].sum(axis=0)
    assert np.allclose(lhs, rhs, rtol=1e-9, atol=1e-9), np.abs(lhs - rhs).max()
    m = ts.merge(got["tree_visits"], got["tree_q"], R, W)
    assert np.array_equal(m["visits"].sum(axis=1), np.full(R, W * S))
    for k in ("q", "visits", "best", "value"):
        assert np.array_equal(m[k], got[k])


PROPS = {"k0_at_root": prop_single_simulation_is_one_step_then_a_rollout,
         "unvisited_last": prop_unvisited_actions_are_tried_in_list_order,
         "last_maximum": prop_ties_go_to_the_first_maximum,
         "backup_from_root": prop_counts_and_means_add_up}


@pytest.mark.parametrize("rule", list(PROPS))
def test_restatement_property(rule):
    PROPS[rule]()


@pytest.mark.parametrize("rule", list(PROPS))
def test_every_rule_is_pinned_by_a_property(rule):
    """One one-token mutation per rule (tree_search_restatement.MUTATIONS; each property's docstring names its own): the
    property that holds for the restatement as written fails for the mutant."""
    assert set(PROPS) == set(ts.MUTATIONS)
    with pytest.raises(AssertionError):
        PROPS[rule](mutate=rule)


def test_restatement_greedy_depth_one_is_the_mean_of_first_rewards():
    """ucb_c = 0 and D = 1: no bonus and no rollout (the children are created all the same, one per (action, observation) seen) —
    V(0, a) is the running mean of the rewards of action a, which for RockSample's integer rewards is exact whatever the
    order of the additions."""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("rock")
    R, W, S = 8, 2, 30
    roots = _reset(o, R)
    got = ts.search(o, roots, R, W, S, 1, .95, 0.0, SEED, 0, 3)
    assert (got["n_nodes"] <= S + 1).all() and (got["sim_tree_steps"] == 1).all() and (got["sim_steps"] == 1).all()
    lists, lens = ol._batch_legal(o, roots)
    for i in range(R * W):
        r = i // W
        for a in set(lists[r, :lens[r]].tolist()):
            st = roots[:, r:r + 1].copy()
            # RockSample's reward does not depend on the sensor draw: any counter gives it
            _, rew, _, _ = o.batch_step(st, np.array([a], np.int32), SEED, 4 * i, 0, auto_reset=False)
            assert got["tree_visits"][i, a] >= 1
            assert got["tree_q"][i, a] == float(rew[0]), (i, a)
    assert (got["tree_visits"].sum(axis=1) == S).all()


def test_restatement_tiger_never_opens_the_tigers_door():
    """Tiger from the true states, R = 64, W = 4, S = 32, D = 4, c = 10: opening the tiger's door pays -20 and ends the
    episode, the other door pays +10 and LISTEN -1 — whatever follows, the tiger's door has the lowest value at the root,
    so the merged `best` is never that door."""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("tiger")
    R, W, S, D = 64, 4, 32, 4
    roots = _reset(o, R)
    got = ts.search(o, roots, R, W, S, D, .95, 10.0, SEED, 0, 11)
    tiger_door = (roots[0] & 1).astype(np.int32)
    assert (got["best"] >= 0).all() and (got["best"] != tiger_door).all()
    assert (got["visits"][np.arange(R), tiger_door] >= W).all()           # every tree did try it
    assert (got["q"][np.arange(R), tiger_door] == -20.0).all()
    assert (got["visits"].sum(axis=1) == W * S).all()
