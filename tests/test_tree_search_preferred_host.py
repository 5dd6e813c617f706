"""The preferred-policy tree search without a GPU: the C ABI's declarations and argument checks, the policy workspace's size,
the kernels' resources, and the contract's CPU restatement (tests/tree_search_preferred_restatement.py) checked against what
such a search must satisfy, on the oracle alone — with the proof that each of its new rules is pinned by one property."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preferred_rollout_restatement as rr  # noqa: E402
import tree_search_preferred_restatement as tp  # noqa: E402
import tree_search_restatement as ts  # noqa: E402

NAMES = ("pomdp_tree_search_preferred_workspace", "pomdp_tree_search_preferred")
BAD = -1


def test_entry_points_are_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    for sym in NAMES:
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in _native.SYMBOLS
        assert hasattr(_native.lib(), sym)
    assert "tree_search_preferred.hip" in _native.UNITS
    assert _native.ABI_VERSION == 15 and _native.lib().pomdp_abi_version() == 15
    body = re.search(r"typedef struct pomdp_tree_policy \{(.*?)\} pomdp_tree_policy;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _native.PlanTreePolicy._fields_]
    assert C.sizeof(_native.PlanTreePolicy) == 56 and _native.PlanTreePolicy.prior_v.offset == 48
    assert C.sizeof(_native.PlanTreeArgs) == 200                              # pomdp_tree_args is what it was
    import inspect
    from gym_pomdp_amd.envs.base import BatchedEnv
    for f in (BatchedEnv.search, BatchedEnv.search_step):
        par = inspect.signature(f).parameters
        assert [par[k].default for k in ("policy", "history", "prior_n", "prior_v")] == ["uniform", None, 0, 0.0]


def _rock_params(num_rocks=8):
    from gym_pomdp_amd import _native
    p = _native.RockParams(size=7, num_rocks=num_rocks, start_x=0, start_y=3)
    for i in range(256):
        p.grid[i] = -1
    for i in range(32):
        p.thr[i] = 1 << 52
    return p


X = 1 << 42                                                                   # a fake "device" address, 16-byte aligned


def _caller(env, params, n_act, R=8, W=4, S=16, D=8):
    """-> call(**overrides of pomdp_tree_args, pol=dict of overrides of pomdp_tree_policy | None, hist=..., bel=...)"""
    from gym_pomdp_amd import _native
    L = _native.lib()
    need = L.pomdp_tree_search_workspace(env, C.byref(params), R * W, S, D)
    pneed = L.pomdp_tree_search_preferred_workspace(env, C.byref(params), R * W)
    assert need > 0

    def call(pol={}, hist={}, bel={}, t0=0, **kw):
        f = dict(env=env, depth=D, params=C.addressof(params), root_state=X, particles=None, n_roots=R, n_particles=0,
                 trees_per_root=W, sims_per_tree=S, discount=.95, ucb_c=1.0, logn=X, workspace=X, workspace_bytes=need,
                 tree_visits=X, tree_q=X, n_nodes=X, sim_ret=None, sim_steps=None, sim_tree_steps=None,
                 out=_native.PlanOut(q=X, visits=X, best=X, value=None, stride=n_act, reserved=0), seed=7, lane0=0, reserved=0)
        f.update(kw)
        args = _native.PlanTreeArgs(**f)
        if pol is None:
            return L.pomdp_tree_search_preferred(C.byref(args), None, t0, None)
        h = dict(size=X, last_action=X, last_ob=X, total_sample=X, total_move=X, move_ok=X, ring=None, head=None, max_size=-1,
                 reserved=0)
        h.update(hist)
        hp = _native.HistoryPtrs(**h)
        b = dict(count=X, measured=X, lkv=X, lkw=X, prob_valuable=X, check_ok=X)
        b.update(bel)
        bp = _native.RockBelief(**b)
        q = dict(belief=C.addressof(bp), history=C.addressof(hp), prev_ob=X, workspace=X, workspace_bytes=pneed, prior_n=0,
                 reserved=0, prior_v=0.0)
        q.update(pol)
        return L.pomdp_tree_search_preferred(C.byref(args), C.byref(_native.PlanTreePolicy(**q)), t0, None)
    return call, need, pneed


def test_bad_arguments_are_refused_before_any_launch():
    """Every check runs on the host: none of these calls reaches the GPU (fake device pointers are never dereferenced)."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    rock = _rock_params()
    call, need, pneed = _caller(0, rock, 13)
    assert pneed == 32 * 8 * 32
    assert L.pomdp_tree_search_preferred(None, None, 0, None) == BAD
    # everything pomdp_tree_search refuses
    for k in ("root_state", "logn", "workspace", "tree_visits", "tree_q", "n_nodes"):
        assert call(**{k: None}) == BAD, k
    assert call(workspace_bytes=need - 1) == call(workspace=X + 8) == BAD
    assert call(lane0=2) == call(n_roots=-1) == call(trees_per_root=0) == call(sims_per_tree=0) == call(depth=-1) == BAD
    for c in (-1.0, float("nan"), float("inf")):
        assert call(ucb_c=c) == BAD, c
    assert call(particles=X, n_particles=6) == call(n_particles=8) == call(env=9) == BAD
    bad_rock = _rock_params()
    bad_rock.size = 99
    assert call(params=C.addressof(bad_rock)) == -2                           # POMDP_E_BADPARAMS
    # the policy's own
    assert call(pol=None) == BAD
    assert call(pol=dict(history=None)) == BAD
    assert call(hist=dict(max_size=5, ring=X, head=X)) == call(hist=dict(max_size=0, ring=X, head=X)) == BAD
    assert call(hist=dict(size=None)) == call(hist=dict(total_move=None)) == call(hist=dict(move_ok=None)) == BAD
    assert call(pol=dict(belief=None)) == call(bel=dict(lkv=None)) == call(pol=dict(prev_ob=None)) == BAD
    assert call(pol=dict(workspace=None)) == call(pol=dict(workspace=X + 8)) == call(pol=dict(workspace_bytes=pneed - 1)) == BAD
    assert call(pol=dict(prior_n=-1)) == call(pol=dict(prior_n=65536)) == BAD
    for v in (float("nan"), float("inf"), -float("inf")):
        assert call(pol=dict(prior_v=v)) == BAD, v
    # W * (S + A * prior_n) > 2^31 - 1: 4 * (16 + 13 * 65535) fits, 2521 * (16 + 13 * 65535) does not (R = 0: no workspace needed)
    assert call(n_roots=0, trees_per_root=2520, pol=dict(prior_n=65535)) == 0
    assert call(n_roots=0, trees_per_root=2521, pol=dict(prior_n=65535)) == BAD
    assert call(n_roots=0) == 0 and call(n_roots=0, pol=dict(workspace=None, workspace_bytes=0)) == 0
    # Tag reads neither the side statistics nor prev_ob nor a workspace
    tag = _native.TagParams(num_opponents=1, obs_cells=29, move_thr=1 << 52, move_gt=0, reserved=0)
    tcall, _, tneed = _caller(1, tag, 5)
    assert tneed == 0
    assert tcall(n_roots=0) == 0
    assert tcall(n_roots=0, pol=dict(belief=None, prev_ob=None, workspace=None, workspace_bytes=0)) == 0
    assert tcall(n_roots=0, hist=dict(total_sample=None, total_move=None, move_ok=None)) == 0
    assert tcall(pol=dict(history=None)) == tcall(hist=dict(max_size=3)) == tcall(pol=dict(prior_n=65536)) == BAD


def test_envs_without_a_policy_forward_or_refuse():
    """Tiger: prior_n == 0 is pomdp_tree_search (pol's pointers are ignored — NULL history included), prior_n > 0 is refused."""
    from gym_pomdp_amd import _native
    tiger = _native.TigerParams(listen_thr=1 << 52)
    call, need, pneed = _caller(3, tiger, 3)
    assert pneed == 0
    assert call(n_roots=0) == 0
    assert call(n_roots=0, pol=dict(history=None, belief=None, prev_ob=None, workspace=None, workspace_bytes=0)) == 0
    assert call(n_roots=0, pol=dict(prior_n=1)) == BAD
    assert call(pol=None) == BAD
    assert call(logn=None, pol=dict(history=None)) == BAD                      # pomdp_tree_search's own refusals still hold
    assert call(workspace_bytes=need - 1) == BAD


def test_policy_workspace_size():
    from gym_pomdp_amd import _native
    L = _native.lib()
    ws = lambda K=8, n=32: L.pomdp_tree_search_preferred_workspace(0, C.byref(_rock_params(K)), n)
    assert ws() == 32 * 8 * 32 and ws(K=15, n=1) == 32 * 15 and ws(n=0) == 0 and ws(n=-1) == 0
    assert [ws(n=n) for n in range(5)] == [n * ws(n=1) for n in range(5)]
    assert L.pomdp_tree_search_preferred_workspace(0, None, 32) == 0
    tag = _native.TagParams(num_opponents=1, obs_cells=29, move_thr=1 << 52, move_gt=0, reserved=0)
    assert L.pomdp_tree_search_preferred_workspace(1, C.byref(tag), 32) == 0
    assert L.pomdp_tree_search_preferred_workspace(3, C.byref(_native.TigerParams(listen_thr=1)), 32) == 0


def test_kernels_keep_nothing_in_scratch_memory_and_tree_search_hip_is_what_it_was():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = kr.collect(units=["tree_search_preferred.hip"])
    names = [r["kernel"] for r in rows]
    assert names and all(k.startswith("tree_preferred_kernel<") for k in names)
    assert not [k for k in names if k.startswith("tree_search_kernel<")]
    assert all("RockEnv" in k or "TagEnv" in k for k in names), names          # the envs has_policy covers, no others
    assert sum("TagEnv" in k for k in names) == 1
    bad = [(r["kernel"], r["scratch"]) for r in rows if r["scratch"] != "0"]
    assert not bad, bad
    old = [r["kernel"] for r in kr.collect(units=["tree_search.hip"])]
    assert sum(1 for k in old if k.startswith("tree_search_kernel<")) == 11 and old.count("tree_merge_kernel") == 1
    assert len(old) == 12 and "tree_merge_kernel" not in names                 # the merge is not duplicated


# ---- the restatement on the oracle alone ------------------------------------------------------------------------------------
SEED = 77


def _roots(name, R, steps=6, root_seed=None, **kw):
    """prepared roots, optionally with constructed statistics; steps=0: one step in, with the history cleared again"""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv(name, **kw)
    st, belief, history, pob, _ = rr.prepare_roots(o, R, max(steps, 1), SEED, 0)
    if steps == 0:
        cleared = ol.HistorySums(o, R)
        history = {f: getattr(cleared, f).copy() for f in history}
    if root_seed is not None:
        belief, history, pob = rr.construct_roots(o, st, 1, belief, history, pob, root_seed)
    return o, st, belief, history, pob


def _after_first_step(o, st, belief, history, pob, R, col, lane0, t):
    """the roots after the tree-mode step `legal list[col]` at counter t: (states, reward, done, belief, history, prev_ob), the
    policy inputs updated as one non-auto-reset step of pomdp_heuristic_steps updates them"""
    from oracle import oracle_lib as ol
    lists, lens = ol._batch_legal(o, st)
    assert (lens > col).all()
    a = lists[:, col].copy()
    bel, hs, p = rr.expand(o, belief, history, pob, R, 1)
    nx = st.copy()
    ob, rew, done, _ = o.batch_step(nx, a, SEED, lane0, t, auto_reset=False)
    if bel is not None:
        bel.update(nx, a, ob, done, auto_reset=False)
    hs.append(p, a, ob, done, auto_reset=False)
    b2 = None if bel is None else {f: getattr(bel, f).copy() for f, _ in ol.Belief.FIELDS}
    h2 = {f: getattr(hs, f).copy() for f in ("size", "last_action", "last_ob", "total_sample", "total_move")}
    return nx, a, rew.astype(np.float64), done != 0, b2, h2, np.ascontiguousarray(ob.astype(np.int32))


def _first_visit_returns(o, st, belief, history, pob, R, D, disc, lane0, t0, sim):
    """what simulation `sim` < len(legal list) of a W = 1 search without priors must return: it takes the sim-th legal action
    at the root (the first unvisited), creates a node and rolls out — r + discount * (the return of a
    pomdp_rollout_preferred simulation of depth D - 1 from the post-step state and the post-step policy inputs at t_s + 1)"""
    t_s = t0 + sim * D
    nx, a, r, done, b2, h2, p2 = _after_first_step(o, st, belief, history, pob, R, sim, lane0, t_s)
    ro = rr.rollout(o, nx, b2, h2, p2, R, 1, 1, D - 1, disc, SEED, lane0, t_s + 1)
    return np.where(done, r, r + np.float64(disc) * ro["ret"]), a


def prop_tree_steps_update_the_private_inputs(mutate=None):
    """W = 1, S = 1: the one simulation's return is its first reward plus discount times a flat preferred rollout from the
    leaf that starts from the root's inputs UPDATED by the tree-mode step.  Tag's roots have empty histories (all five
    actions preferred) that the step makes non-empty; RockSample's constructed roots sit at the policy's thresholds.
    Mutation that fails it: `upd = active` -> `active & ~in_tree` (no_tree_update)."""
    for name, root_seed in (("tag", None), ("rock", 1)):
        R, D, disc, lane0, t0 = 24, 9, .95, 8, 1000
        o, st, belief, history, pob = _roots(name, R, steps=0 if name == "tag" else 6, root_seed=root_seed)
        got = tp.search(o, st, belief, history, pob, R, 1, 1, D, disc, 1.0, SEED, lane0, t0, mutate=mutate)
        want, a = _first_visit_returns(o, st, belief, history, pob, R, D, disc, lane0, t0, 0)
        assert np.array_equal(got["sim_ret"][0], want), name
        assert np.array_equal(got["tree_q"][np.arange(R), a], want) and (got["tree_visits"].sum(axis=1) == 1).all()


def prop_every_simulation_starts_from_the_roots_inputs(mutate=None):
    """W = 1, S = 2: simulation 1 takes the second legal action at the root and rolls out from the ROOT's inputs updated by
    that one step — not from what simulation 0 left in the private column.
    Mutation that fails it: `mutate != "no_refill"` dropped, so that only simulation 0 refills (no_refill)."""
    for name, root_seed in (("tag", None), ("rock", 1)):
        R, D, disc, lane0, t0 = 24, 9, .95, 8, 1000
        o, st, belief, history, pob = _roots(name, R, steps=0 if name == "tag" else 6, root_seed=root_seed)
        got = tp.search(o, st, belief, history, pob, R, 1, 2, D, disc, 1.0, SEED, lane0, t0, mutate=mutate)
        for sim in (0, 1):
            want, _ = _first_visit_returns(o, st, belief, history, pob, R, D, disc, lane0, t0, sim)
            assert np.array_equal(got["sim_ret"][sim], want), (name, sim)


def prop_fallback_nodes_get_priors_too(mutate=None):
    """RockSample(7,8) from constructed roots (a sixth of them cornered, which is what reaches the legal fallback): nodes whose
    P(h) was the fallback exist, and every node that got priors got them for at least one action.
    Mutation that fails it: `Pl_prior = Pl` -> `[]` on fallback (no_fallback_priors)."""
    R, W, S, D = 12, 4, 33, 10
    o, st, belief, history, pob = _roots("rock", R, root_seed=1)
    got = tp.search(o, st, belief, history, pob, R, W, S, D, .95, 1.0, SEED, 0, 100, prior_n=3, prior_v=5.0, mutate=mutate)
    assert got["stats"]["prior_from_fallback"] >= 1
    assert min(min(p) for p in got["prior_sizes"]) >= 1


def prop_visits_are_simulations_plus_the_roots_priors(mutate=None):
    """prior_n > 0: sum_a tree_visits is the number of simulations that took a step plus prior_n * |P(0)| — the root's priors
    are set once, by simulation 0, and the backups run on top of them; the merge adds the trees' own.
    Mutation that fails it: `s == 0` -> `s == 0 or ...every simulation` (root_priors_every_sim)."""
    for name, root_seed in (("tag", 3), ("rock", 1)):
        R, W, S, D, pn = 6, 2, 20, 6, 3
        o, st, belief, history, pob = _roots(name, R, root_seed=root_seed)
        got = tp.search(o, st, belief, history, pob, R, W, S, D, .95, 5.0, SEED, 4, 7, prior_n=pn, prior_v=5.0, mutate=mutate)
        assert (got["root_prior_size"] >= 1).all()
        want = (got["sim_steps"] > 0).sum(axis=0) + pn * got["root_prior_size"]
        assert np.array_equal(got["tree_visits"].sum(axis=1), want), name
        assert np.array_equal(got["visits"].sum(axis=1), want.reshape(R, W).sum(axis=1))
        assert (got["n_nodes"] <= S + 1).all()


def prop_nh_counts_the_priors(mutate=None):
    """Tag from empty histories, D = 1, prior_n = 1, prior_v = -100, c = 10^6: all five actions start with N = 1, so every
    selection is by UCB1 with Nh = 5 + s, and the bonus c * sqrt(log(Nh) / N) sends each of the first five simulations to an
    action with N still 1: after S = 5 every action has exactly one real visit.  With Nh counted without the priors the first
    selection reads logn[0] (a NaN bonus) and the second log(1) = 0: no bonus, and the action already visited, whose value
    rose above the prior (Tag's rewards are -1, -10 and +10), is taken again.
    Mutation that fails it: Nh minus the node's priors (nh_without_priors)."""
    R = 8
    o, st, belief, history, pob = _roots("tag", R, steps=0)
    assert (history["size"] == 0).all()
    got = tp.search(o, st, belief, history, pob, R, 1, 5, 1, .95, 1e6, SEED, 0, 0, prior_n=1, prior_v=-100.0, mutate=mutate)
    assert (got["tree_visits"] == 2).all()


PROPS = {"no_refill": prop_every_simulation_starts_from_the_roots_inputs,
         "no_tree_update": prop_tree_steps_update_the_private_inputs,
         "no_fallback_priors": prop_fallback_nodes_get_priors_too,
         "root_priors_every_sim": prop_visits_are_simulations_plus_the_roots_priors,
         "nh_without_priors": prop_nh_counts_the_priors}


@pytest.mark.parametrize("rule", list(PROPS))
def test_restatement_property(rule):
    PROPS[rule]()


@pytest.mark.parametrize("rule", list(PROPS))
def test_every_rule_is_pinned_by_a_property(rule):
    """One one-token mutation per new rule (tree_search_preferred_restatement.MUTATIONS; each property's docstring names its
    own): the property that holds for the restatement as written fails for the mutant."""
    assert set(PROPS) == set(tp.MUTATIONS)
    with pytest.raises(AssertionError):
        PROPS[rule](mutate=rule)


def test_where_the_preferred_list_is_the_legal_list_it_is_the_uniform_search():
    """prior_n == 0 on roots whose preferred list equals the legal list at every step reached: Tag from an empty history with
    D = 1 (all five actions, which is Tag's legal list) — the restatement equals tree_search_restatement.search."""
    R, W, S = 10, 4, 12
    o, st, belief, history, pob = _roots("tag", R, steps=0)
    assert (history["size"] == 0).all()
    got = tp.search(o, st, belief, history, pob, R, W, S, 1, .95, 1.0, SEED, 4, 9)
    want = ts.search(o, st, R, W, S, 1, .95, 1.0, SEED, 4, 9)
    for k in ("tree_visits", "tree_q", "n_nodes", "sim_ret", "sim_steps", "sim_tree_steps", "q", "visits", "best", "value"):
        assert np.array_equal(got[k], want[k]), k
    assert got["stats"]["empty_history_all_five"] == R * W * S


def test_counters_see_every_branch_on_constructed_roots():
    """what the GPU test relies on, at its largest row shape: from constructed roots the restatement reaches every RockSample
    counter, the two new ones included, and never a NaN probability"""
    R, W, S, D = 12, 4, 33, 10
    o, st, belief, history, pob = _roots("rock", R, root_seed=1)
    got = tp.search(o, st, belief, history, pob, R, W, S, D, .95, 1.0, SEED, 0, 100, prior_n=3, prior_v=5.0)
    s = got["stats"]
    for c in rr.ROCK_COUNTERS + ("recheck_across_sims", "prior_from_fallback"):
        assert s[c] >= 1, (c, s)
    assert s["nan_prob"] == 0
