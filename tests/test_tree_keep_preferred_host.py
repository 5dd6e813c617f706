"""The preferred-policy search resumed from kept trees, without a GPU: the C ABI's declaration and argument checks, the new
kernel's resources, the new pool helpers under the host sanitizers (tools/tree_keep_preferred_hostcheck.cpp, a stand-alone
program), and the contract's CPU restatement (tests/tree_keep_preferred_restatement.py) checked on the oracle alone — the
anchor against tree_search_preferred_restatement, and the proof that each new rule is pinned by one property.

It also holds what test_gpu_tree_keep_preferred.py shares: the rows, the priors, and play_on_the_oracle(), the GPU test's real
steps on the oracle alone, which is how the rows' seeds, ucb_c and REACHED table were chosen."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preferred_rollout_restatement as rr  # noqa: E402
import tree_keep_preferred_restatement as kp  # noqa: E402
import tree_keep_restatement as tk  # noqa: E402
import tree_search_preferred_restatement as tp  # noqa: E402
import tree_search_restatement as ts  # noqa: E402

SEED = 4242                                                    # test_gpu_preferred.make's
ENVS = [("rock", {}), ("rock", dict(board_size=15, num_rocks=15)), ("stochrock", {}), ("tag", {})]
ENV_NAMES = ["rock7-8", "rock15-15", "stochrock", "tag"]
PREP, ROOT_SEED = 6, 1                                         # test_gpu_tree_search_preferred.py's roots
DISCOUNT = .95
UCB = {"rock": 20.0, "stochrock": 20.0, "tag": 10.0}
PRIORS = [(0, 0.0), (3, 5.0), (1, -20.0)]
PRIOR_NAMES = ["no-priors", "n3-v5", "n1-v-20"]
# (R, W, lane_offset, S, D, C, P, real steps), the priors the row runs under
ROWS = [((6, 4, 0, 33, 10, 67, 0, 4), (0, 1, 2)),     # kept subtrees with priors, Nh past S + A * prior_n; no pool fills
        ((6, 4, 0, 33, 10, 34, 0, 4), (1,)),          # the full-pool branch: nothing is primed or written there
        ((2, 16, 0, 33, 10, 67, 8, 3), (1,)),         # particles: an empty tree's node 0 gets its priors from a particle
        ((70, 4, 0, 33, 2, 67, 0, 3), (1, 2)),        # two workgroups, the second partial; D = 2: nodes made on a simulation's last step
        ((5, 1, 4, 1, 1, 3, 0, 3), (1, 2)),           # W = 1 at a lane offset; D = 1: every kept root arrives unprimed
        ((3, 4, 0, 9, 5, 1, 0, 3), (1,)),             # C = 1
        ((3, 4, 0, 2, 0, 5, 0, 1), (0, 1)),           # D = 0: no priors, best == -1
        ((6, 4, 8, 9, 6, 19, 0, 3), (1,))]            # a shard at lane_offset 8 against the unsharded restatement's lanes
ROW_NAMES = ["6x4-S33-D10-C67", "6x4-S33-D10-C34", "2x16-S33-D10-C67-P8", "70x4-S33-D2-C67", "5x1@4-S1-D1-C3", "3x4-S9-D5-C1", "3x4-S2-D0",
             "6x4@8-S9-D6-C19"]
# What the restatement reaches per env, over the rows and priors above (play_on_the_oracle: seed 4242, six heuristic steps of
# warm-up, constructed roots of seed 1, the ucb_c above), found by running it on the oracle and asserted on the restatement's
# side by the GPU test: "late" late_priors >= 1, "reused" kept_primed_reused >= 1, "kept8" a kept tree of at least 8 nodes,
# "full" a full pool, "ended" a lane whose episode a real step ends, "nomatch" a live lane's tree without the real step's
# child, "recheck" recheck_across_sims >= 1 in a search that resumed a kept RockSample tree.
REACHED = {"rock7-8": {"late", "reused", "kept8", "full", "nomatch", "recheck"},
           "rock15-15": {"late", "reused", "full", "nomatch", "recheck"},
           "stochrock": {"late", "reused", "kept8", "full", "nomatch", "recheck"},
           "tag": {"late", "reused", "kept8", "full", "ended", "nomatch"}}
BRANCHES = {"late", "reused", "kept8", "full", "ended", "nomatch", "recheck"}


def new_seen():
    return dict(late=0, reused=0, kept=0, full=0, ended=0, nomatch=0, recheck=0, nh=0, sizes=[])


def observe(seen, want, resumed, trees_after, best, dn, was_done, R, W):
    """one real step's account: `want` the restatement's search, resumed: some tree was non-empty before it, trees_after: the
    trees after the advance"""
    st = want["stats"]
    seen["late"] += st["late_priors"]
    seen["reused"] += st["kept_primed_reused"]
    seen["full"] += int(want["full"].sum())
    seen["recheck"] += st["recheck_across_sims"] if resumed else 0
    seen["nh"] = max(seen["nh"], max(t.Nh[0] for t in want["trees"]))
    seen["sizes"].append(int(want["n_nodes"].max()))
    sizes = tk.n_nodes_of(trees_after).reshape(R, W)
    live = ~dn & (best >= 0)
    seen["kept"] = max(seen["kept"], int(sizes.max()))
    seen["nomatch"] += int((sizes[live] == 0).sum())
    seen["ended"] += int((dn & ~was_done).sum())
    assert (sizes[~live] == 0).all()                                      # ended lanes and best == -1 lanes end up empty
    return seen


def reached_of(seen):
    return {b for b in BRANCHES if (seen["kept"] >= 8 if b == "kept8" else seen[b] >= 1)}


def play_on_the_oracle(ei, ri, pi, mutate=None, steps=None):
    """search_step(policy="preferred", history=, tree=) over the row's real steps, on the oracle alone: the roots of
    test_gpu_tree_search_preferred.py (rr.prepare_roots, rr.construct_roots), then per real step the restatement's search, the
    oracle's step of the best actions, the side statistics and the history append, and tk.advance.  True states only (P == 0).
    -> (seen, the per-step search dicts)"""
    from oracle import oracle_lib as ol
    env, kw = ENVS[ei]
    (R, W, lane_offset, S, D, Cn, P, n_steps), _ = ROWS[ri]
    assert P == 0
    n_steps = n_steps if steps is None else steps
    prior_n, prior_v = PRIORS[pi]
    o = ol.OracleEnv(env, **kw)
    st, belief, history, pob, done = rr.prepare_roots(o, R, PREP, SEED, lane_offset)
    belief, history, pob = rr.construct_roots(o, st, 1, belief, history, pob, ROOT_SEED)
    frozen = (np.asarray(done) != 0).astype(np.uint8)
    t = PREP + 1
    logn = kp.log_table(n_steps, S, o.n_actions, prior_n)
    trees, seen, res = None, new_seen(), []
    for _ in range(n_steps):
        resumed = trees is not None and any(x is not None for x in trees)
        want = kp.search(o, st, belief, history, pob, R, W, S, D, DISCOUNT, UCB[env], SEED, lane_offset * W, t, trees=trees, C=Cn,
                         logn=logn, prior_n=prior_n, prior_v=prior_v, nthreads=ol.max_threads(), mutate=mutate)
        res.append(want)
        t += S * D
        best = want["best"]
        real = st.copy()
        wob, wrew, wdone, _ = o.batch_step(real, best, SEED, lane_offset, t, auto_reset=False, done=frozen.copy())
        t += 1
        bel, hs, p = rr.expand(o, belief, history, pob, R, 1)
        live = frozen == 0
        if bel is not None:
            bel.update(real, np.where(live, best, 0).astype(np.int32), np.where(live, wob, 0).astype(np.int32),
                       np.where(live, wdone, 1).astype(np.uint8), auto_reset=False)
            belief = {f: getattr(bel, f).copy() for f, _ in ol.Belief.FIELDS}
        hs.append(p, best.astype(np.int32), wob.astype(np.int32), wdone, auto_reset=False)
        history = {f: getattr(hs, f).copy() for f in history}
        pob = np.ascontiguousarray(wob.astype(np.int32))
        dn = wdone != 0
        trees = tk.advance(want["trees"], W, best, wob.astype(np.int32), dn.astype(np.uint8))
        observe(seen, want, resumed, trees, best, dn, frozen != 0, R, W)
        st, frozen = real, wdone.astype(np.uint8) | frozen
    return seen, res


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
NAME = "pomdp_tree_search_preferred_resume"
X, B_, N1 = 1 << 42, 1 << 41, 1 << 44                                     # fake "device" addresses, 16-byte aligned
BAD = -1


def test_the_entry_point_is_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, hdr) and NAME in _native.SYMBOLS and hasattr(_native.lib(), NAME)
    assert "tree_keep_preferred.hip" in _native.UNITS
    assert _native.ABI_VERSION == 15 and _native.lib().pomdp_abi_version() == 15       # a new entry point only
    assert "The uniform search only" not in hdr
    assert C.sizeof(_native.PlanTreeKeep) == 40 and C.sizeof(_native.PlanTreeArgs) == 200 and C.sizeof(_native.PlanTreePolicy) == 56


def _rock_params(num_rocks=8):
    from gym_pomdp_amd import _native
    p = _native.RockParams(size=7, num_rocks=num_rocks, start_x=0, start_y=3)
    for i in range(256):
        p.grid[i] = -1
    for i in range(32):
        p.thr[i] = 1 << 52
    return p


def _caller(env, params, n_act, R=8, W=4, S=16, D=8, Cn=9):
    from gym_pomdp_amd import _native
    L = _native.lib()
    need = L.pomdp_tree_keep_workspace(env, C.byref(params), R * W, Cn, D)
    pneed = L.pomdp_tree_search_preferred_workspace(env, C.byref(params), R * W)
    assert need > 0

    def call(pol={}, hist={}, bel={}, keep={}, t0=0, **kw):
        f = dict(env=env, depth=D, params=C.addressof(params), root_state=X, particles=None, n_roots=R, n_particles=0,
                 trees_per_root=W, sims_per_tree=S, discount=.95, ucb_c=1.0, logn=X, workspace=None, workspace_bytes=0,
                 tree_visits=X, tree_q=X, n_nodes=X, sim_ret=None, sim_steps=None, sim_tree_steps=None,
                 out=_native.PlanOut(q=X, visits=X, best=X, value=None, stride=n_act, reserved=0), seed=7, lane0=0, reserved=0)
        f.update(kw)
        args = _native.PlanTreeArgs(**f)
        h = dict(size=X, last_action=X, last_ob=X, total_sample=X, total_move=X, move_ok=X, ring=None, head=None, max_size=-1,
                 reserved=0)
        h.update(hist)
        hp = _native.HistoryPtrs(**h)
        b = dict(count=X, measured=X, lkv=X, lkw=X, prob_valuable=X, check_ok=X)
        b.update(bel)
        bp = _native.RockBelief(**b)
        q = dict(belief=C.addressof(bp), history=C.addressof(hp), prev_ob=X, workspace=X, workspace_bytes=pneed, prior_n=0,
                 reserved=0, prior_v=0.0)
        if pol is not None:
            q.update(pol)
        k = dict(workspace=B_, workspace_bytes=need, n_nodes=N1, node_capacity=Cn, logn_len=S + 1 + n_act * q["prior_n"])
        if keep is not None:
            k.update(keep)
        return getattr(L, NAME)(C.byref(args), None if pol is None else C.byref(_native.PlanTreePolicy(**q)),
                                None if keep is None else C.byref(_native.PlanTreeKeep(**k)), t0, None)
    return call, need, pneed


def test_bad_arguments_are_refused_before_any_launch():
    """Every check runs on the host: none of these calls reaches the GPU (fake device pointers are never dereferenced)."""
    from gym_pomdp_amd import _native
    rock = _rock_params()
    call, need, pneed = _caller(0, rock, 13)
    assert getattr(_native.lib(), NAME)(None, None, None, 0, None) == BAD
    assert call(pol=None) == call(keep=None) == BAD
    # what pomdp_tree_search_preferred refuses, its tree workspace and (S + 1) * A rules aside
    for k in ("root_state", "logn", "tree_visits", "tree_q", "n_nodes"):
        assert call(**{k: None}) == BAD, k
    assert call(lane0=2) == call(n_roots=-1) == call(trees_per_root=0) == call(sims_per_tree=0) == call(depth=-1) == BAD
    for c in (-1.0, float("nan"), float("inf")):
        assert call(ucb_c=c) == BAD, c
    assert call(particles=X, n_particles=6) == call(n_particles=8) == call(env=9) == BAD
    bad_rock = _rock_params()
    bad_rock.size = 99
    assert call(params=C.addressof(bad_rock)) == -2                           # POMDP_E_BADPARAMS
    assert call(pol=dict(history=None)) == BAD
    assert call(hist=dict(max_size=5, ring=X, head=X)) == call(hist=dict(size=None)) == call(hist=dict(move_ok=None)) == BAD
    assert call(pol=dict(belief=None)) == call(bel=dict(lkv=None)) == call(pol=dict(prev_ob=None)) == BAD
    assert call(pol=dict(workspace=None)) == call(pol=dict(workspace=X + 8)) == call(pol=dict(workspace_bytes=pneed - 1)) == BAD
    assert call(pol=dict(prior_n=-1)) == call(pol=dict(prior_n=65536)) == BAD
    for v in (float("nan"), float("inf"), -float("inf")):
        assert call(pol=dict(prior_v=v)) == BAD, v
    # what pomdp_tree_search_resume refuses about k
    assert call(keep=dict(workspace=None)) == call(keep=dict(n_nodes=None)) == call(keep=dict(workspace=B_ + 8)) == BAD
    assert call(keep=dict(workspace_bytes=need - 1)) == call(keep=dict(node_capacity=0)) == BAD
    assert call(keep=dict(node_capacity=(1 << 31) // 13 + 1, workspace_bytes=1 << 60)) == BAD
    assert call(keep=dict(logn_len=1)) == call(keep=dict(logn_len=-5)) == BAD
    # logn_len - 1 < A * prior_n + 1: a primed node's Nh must index the table
    assert call(n_roots=0, pol=dict(prior_n=3), keep=dict(logn_len=13 * 3 + 2)) == 0
    assert call(n_roots=0, pol=dict(prior_n=3), keep=dict(logn_len=13 * 3 + 1)) == BAD
    # W * (logn_len - 1) > 2^31 - 1
    assert call(n_roots=0, keep=dict(logn_len=(1 << 31) // 4)) == 0
    assert call(n_roots=0, keep=dict(logn_len=(1 << 31) // 4 + 1)) == BAD
    # a->workspace is ignored; S may exceed C - 1 (S = 16, C = 9); n_roots == 0 needs no workspace
    assert call(n_roots=0) == 0 and call(n_roots=0, pol=dict(workspace=None, workspace_bytes=0), keep=dict(workspace=None, workspace_bytes=0)) == 0
    tag = _native.TagParams(num_opponents=1, obs_cells=29, move_thr=1 << 52, move_gt=0, reserved=0)
    tcall, _, tneed = _caller(1, tag, 5)
    assert tneed == 0 and tcall(n_roots=0, pol=dict(belief=None, prev_ob=None, workspace=None, workspace_bytes=0)) == 0
    assert tcall(pol=dict(history=None)) == tcall(hist=dict(max_size=3)) == BAD


def test_envs_without_a_policy_forward_or_refuse():
    """Tiger: prior_n == 0 is pomdp_tree_search_resume (pol's pointers ignored), prior_n > 0 is refused"""
    from gym_pomdp_amd import _native
    call, need, pneed = _caller(3, _native.TigerParams(listen_thr=1 << 52), 3)
    assert pneed == 0 and call(n_roots=0) == 0
    assert call(n_roots=0, pol=dict(history=None, belief=None, prev_ob=None, workspace=None, workspace_bytes=0)) == 0
    assert call(n_roots=0, pol=dict(prior_n=1)) == BAD
    assert call(pol=None) == BAD
    assert call(logn=None, pol=dict(history=None)) == BAD                      # pomdp_tree_search_resume's own refusals still hold
    assert call(keep=dict(workspace_bytes=need - 1), pol=dict(history=None)) == BAD


def test_the_new_kernel_keeps_nothing_in_scratch_memory_and_the_old_units_are_what_they_were():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = kr.collect(units=["tree_keep_preferred.hip"])
    names = [r["kernel"] for r in rows]
    assert names and all(k.startswith("tree_resume_preferred_kernel<") for k in names), names
    assert all("RockEnv" in k or "TagEnv" in k for k in names) and sum("TagEnv" in k for k in names) == 1
    assert not [(r["kernel"], r["scratch"]) for r in rows if r["scratch"] != "0"]
    print(rows)
    old = [r["kernel"] for r in kr.collect(units=["tree_keep.hip"])]
    assert sum(1 for k in old if k.startswith("tree_resume_kernel<")) == 11 and old.count("tree_advance_kernel") == 1 and len(old) == 12


def test_the_new_pool_helpers_under_the_host_sanitizers(tmp_path):
    """tools/tree_keep_preferred_hostcheck.cpp: its own main, tree_keep.hip.h included as it is, pools of exactly the advertised
    bytes; built with g++ -fsanitize=address,undefined and run as a child process."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "tree_keep_preferred_hostcheck")
    cc = subprocess.run([gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-o", exe,
                         os.path.join(REPO, "tools", "tree_keep_preferred_hostcheck.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", cc.stderr):
        pytest.skip("g++ has no sanitizer runtime")
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "tree_keep_preferred_hostcheck: ok" in run.stdout


# ---- the restatement on the oracle alone ------------------------------------------------------------------------------------
def _roots(name, R, steps=6, root_seed=None, **kw):
    from oracle import oracle_lib as ol
    o = ol.OracleEnv(name, **kw)
    st, belief, history, pob, _ = rr.prepare_roots(o, R, steps, SEED, 0)
    if root_seed is not None:
        belief, history, pob = rr.construct_roots(o, st, 1, belief, history, pob, root_seed)
    return o, st, belief, history, pob


TEN = ("tree_visits", "tree_q", "n_nodes", "sim_ret", "sim_steps", "sim_tree_steps", "q", "visits", "best", "value")


@pytest.mark.parametrize("pi", range(3), ids=PRIOR_NAMES)
@pytest.mark.parametrize("name,kw,D", [("rock", {}, 10), ("tag", {}, 10), ("rock", {}, 1), ("tag", {}, 0)],
                         ids=["rock-D10", "tag-D10", "rock-D1", "tag-D0"])
def test_resume_from_empty_equals_the_preferred_search(name, kw, D, pi):
    """the anchor: empty trees, C = S + 1, logn_len = S + 1 + A * prior_n — every output of tp.search, bit for bit, for every D"""
    R, W, S = 6, 4, 20
    o, st, belief, history, pob = _roots(name, R, root_seed=1, **kw)
    pn, pv = PRIORS[pi]
    want = tp.search(o, st, belief, history, pob, R, W, S, D, .95, UCB[name], SEED, 4, 100, prior_n=pn, prior_v=pv)
    got = kp.search(o, st, belief, history, pob, R, W, S, D, .95, UCB[name], SEED, 4, 100, prior_n=pn, prior_v=pv)
    for k in TEN:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(got["root_prior_size"], want["root_prior_size"]) and not got["full"].any()
    for c in tp.COUNTERS:
        assert got["stats"][c] == want["stats"][c], c
    assert got["stats"]["late_priors"] == 0 and got["stats"]["kept_primed_reused"] == 0
    if D == 0:
        assert all(t.Nh == [0] for t in got["trees"])                         # nothing is primed


def _tag_from_empty_histories(R):
    from oracle import oracle_lib as ol
    o, st, belief, history, pob = _roots("tag", R, steps=1)
    cleared = ol.HistorySums(o, R)
    return o, st, belief, {f: getattr(cleared, f).copy() for f in history}, pob


def _visits_at_the_root(t):
    return int(t.N[0].sum())


def prop_a_kept_root_is_not_primed_again(mutate=None):
    """Tag and RockSample under priors (3, 5.0): a second search over the trees the first one left — node 0 kept as it is —
    adds its backups on top of what node 0 holds: sum_a N(0, a) grows by exactly the simulations that took a step, and Nh with
    it.  Mutation that fails it: the test `Nh == 0` also passes for a kept root at its first step (reprime_kept_root)."""
    import copy
    for name, root_seed in (("tag", 3), ("rock", 1)):
        R, W, S, D, pn = 6, 2, 12, 6, 3
        o, st, belief, history, pob = _roots(name, R, root_seed=root_seed)
        logn = kp.log_table(2, S, o.n_actions, pn)
        first = kp.search(o, st, belief, history, pob, R, W, S, D, .95, UCB[name], SEED, 4, 7, C=40, logn=logn, prior_n=pn, prior_v=5.0)
        before = [(_visits_at_the_root(t), t.Nh[0]) for t in first["trees"]]
        assert all(nh == n and n > S for n, nh in before)
        second = kp.search(o, st, belief, history, pob, R, W, S, D, .95, UCB[name], SEED, 4, 7 + S * D, trees=copy.deepcopy(first["trees"]),
                           C=40, logn=logn, prior_n=pn, prior_v=5.0, mutate=mutate)
        took = (second["sim_steps"] > 0).sum(axis=0)
        for i, t in enumerate(second["trees"]):
            assert (_visits_at_the_root(t), t.Nh[0]) == (before[i][0] + took[i], before[i][1] + took[i]), (name, i)
        assert second["stats"]["kept_primed_reused"] == int(took.sum()) and second["stats"]["late_priors"] == 0


def prop_a_kept_unprimed_node_is_primed_by_the_first_simulation_that_stands_on_it(mutate=None):
    """Tag, W = 1, S = 1, D = 1 (row 4's shape): the one simulation creates its node on its last step, so the node has no
    priors and Nh == 0.  Advanced under that very (action, observation) it is the new root, and the next search's simulation 0
    primes it from ITS P(0) before selecting: Nh(0) == prior_n * |P(0)| + 1 afterwards, and late_priors counts every tree.
    Mutation that fails it: a kept node is never primed (never_prime_kept)."""
    R, pn = 8, 3
    o, st, belief, history, pob = _roots("tag", R, root_seed=3)
    logn = kp.log_table(2, 1, o.n_actions, pn)
    first = kp.search(o, st, belief, history, pob, R, 1, 1, 1, .95, 10.0, SEED, 4, 7, C=3, logn=logn, prior_n=pn, prior_v=5.0)
    keys = [list(t.children[0]) for t in first["trees"]]
    assert all(len(k) == 1 for k in keys) and all(t.Nh[1] == 0 and t.Nh[0] > 0 for t in first["trees"])
    trees = tk.advance(first["trees"], 1, np.array([k[0][0] for k in keys]), np.array([k[0][1] for k in keys]))
    assert all(len(t.N) == 1 and t.Nh[0] == 0 for t in trees)
    second = kp.search(o, st, belief, history, pob, R, 1, 1, 1, .95, 10.0, SEED, 4, 8, trees=trees, C=3, logn=logn, prior_n=pn,
                       prior_v=5.0, mutate=mutate)
    assert [t.Nh[0] for t in second["trees"]] == [pn * int(k) + 1 for k in second["root_prior_size"]]
    assert [_visits_at_the_root(t) for t in second["trees"]] == [pn * int(k) + 1 for k in second["root_prior_size"]]
    assert second["stats"]["late_priors"] == R and (second["root_prior_size"] >= 1).all()


def prop_a_full_pool_primes_nothing(mutate=None):
    """C = 1 under priors: every simulation that survives its first step meets a full pool and rolls out without a node; the
    root keeps its priors and every backup, so sum_a N(0, a) == prior_n * |P(0)| + the simulations that took a step.
    Mutation that fails it: the step after a full pool primes the node the lane stands on — the root, wiping its statistics
    (prime_on_full_pool)."""
    for name, root_seed in (("tag", 3), ("rock", 1)):
        R, W, S, D, pn = 6, 2, 12, 6, 3
        o, st, belief, history, pob = _roots(name, R, root_seed=root_seed)
        got = kp.search(o, st, belief, history, pob, R, W, S, D, .95, UCB[name], SEED, 4, 7, C=1, prior_n=pn, prior_v=5.0, mutate=mutate)
        assert got["full"].sum() >= R * W and (got["n_nodes"] == 1).all()
        want = (got["sim_steps"] > 0).sum(axis=0) + pn * got["root_prior_size"]
        assert np.array_equal(got["tree_visits"].sum(axis=1), want), name


def prop_nh_is_clamped_to_the_tables_last_entry(mutate=None):
    """Tag from empty histories, D = 1, W = 1, prior_n = 1 on all five actions: the selection of simulation s reads
    logn[5 + s], so a table of 5 + S entries is read up to its LAST entry by simulation S - 1 and never clamped.  With that
    entry replaced by 10^12 the last selection goes by the visit counts alone instead of the values, and some root's visits
    change: the entry is read.
    Mutation that fails it: Nh clamped one entry short, so that the last entry is never read (nh_clamp_short)."""
    R, S, pn = 16, 7, 1
    o, st, belief, history, pob = _tag_from_empty_histories(R)
    table = ts.log_table(5 * pn + S - 1)
    assert len(table) == 5 * pn + S
    loud = table.copy()
    loud[-1] = 1e12
    run = lambda logn: kp.search(o, st, belief, history, pob, R, 1, S, 1, .95, .01, SEED, 0, 0, C=S + 1, logn=logn, prior_n=pn,
                                 prior_v=-100.0, mutate=mutate)
    x, y, z = run(table), run(loud), run(kp.log_table(3, S, 5, pn))
    assert np.array_equal(x["tree_visits"], z["tree_visits"])                 # a longer table changes nothing: no clamp was hit
    assert not np.array_equal(x["tree_visits"], y["tree_visits"])


PROPS = {"reprime_kept_root": prop_a_kept_root_is_not_primed_again,
         "never_prime_kept": prop_a_kept_unprimed_node_is_primed_by_the_first_simulation_that_stands_on_it,
         "prime_on_full_pool": prop_a_full_pool_primes_nothing,
         "nh_clamp_short": prop_nh_is_clamped_to_the_tables_last_entry}


@pytest.mark.parametrize("rule", list(PROPS))
def test_restatement_property(rule):
    PROPS[rule]()


@pytest.mark.parametrize("rule", list(PROPS))
def test_every_new_rule_is_pinned_by_a_property(rule):
    """One one-token mutation per new rule (tree_keep_preferred_restatement.MUTATIONS; each property's docstring names its
    own): the property that holds for the restatement as written fails for the mutant."""
    assert set(PROPS) == set(kp.MUTATIONS)
    with pytest.raises(AssertionError):
        PROPS[rule](mutate=rule)


# ---- what the GPU test relies on ---------------------------------------------------------------------------------------------
def test_every_branch_is_reached_by_some_env():
    assert set.union(*REACHED.values()) == BRANCHES
    assert "recheck" in REACHED["rock7-8"] and {"late", "reused"} <= REACHED["tag"]


@pytest.mark.parametrize("ei,ri,pi,branches", [(3, 3, 1, {"late", "reused", "ended"}), (3, 1, 1, {"full", "kept8"}),
                                               (0, 4, 2, {"late"}), (0, 1, 1, {"full", "nomatch", "recheck", "reused"})],
                         ids=["tag-D2", "tag-C34", "rock7-8-D1", "rock7-8-C34"])
def test_the_rows_reach_their_branches_on_the_oracle(ei, ri, pi, branches):
    """play_on_the_oracle on four of the GPU test's cases: the branches the REACHED table promises for them"""
    seen, _ = play_on_the_oracle(ei, ri, pi)
    assert branches <= reached_of(seen) and branches <= REACHED[ENV_NAMES[ei]], seen
