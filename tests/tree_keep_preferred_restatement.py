"""CPU restatement of the preferred-policy search resumed from kept trees (include/pomdp_hip.h:
pomdp_tree_search_preferred_resume), written from the header's words on top of tree_search_preferred_restatement (the private
policy column, the lists, the counters) and tree_keep_restatement (KTree with its stored Nh, the pool of C nodes, the clamped
log table, advance()), both imported unchanged.  A tree is a tk.KTree whose nodes may carry priors — priors are stored values,
N, V and Nh, so tk.advance and tk.canon handle them as they are — and None stands for an empty tree.  Shared by
test_tree_keep_preferred_host.py and test_gpu_tree_keep_preferred.py.

The one new rule: an active lane about to choose at a node h of its pool — in tree mode before the selection, or at the first
rollout step after creating h — first lays priors on h from this step's P(h) when h's stored Nh is 0.

search() counts tree_search_preferred_restatement's COUNTERS and two of its own:
  late_priors          kept nodes primed in a later search than the one that created them
  kept_primed_reused   simulations that select at a kept node whose Nh was already > 0 (prior_n > 0 only)

`mutate` exists for the host test's self-check only: each value breaks one of the NEW rules by one token."""
import numpy as np

import preferred_rollout_restatement as rr
import tree_keep_restatement as tk
import tree_search_preferred_restatement as tp
import tree_search_restatement as ts
from oracle import oracle_lib as ol
from oracle.philox_ref import stream_words

M64 = ts.M64
MUTATIONS = ("reprime_kept_root", "never_prime_kept", "prime_on_full_pool", "nh_clamp_short")
COUNTERS = tp.COUNTERS + ("late_priors", "kept_primed_reused")


def log_table(searches, S, A, prior_n):
    """a table no Nh of `searches` consecutive searches is clamped by: searches * S + A * prior_n + 1 entries"""
    return ts.log_table(searches * S + A * prior_n)


def set_priors(tree, h, P, prior_n, prior_v):
    """N = prior_n, V = prior_v on P, 0 and 0.0 elsewhere, Nh = sum_a N(h, a) = prior_n * (the distinct actions of P:
    RockSample(15,15)'s legal list, the fallback, names one CHECK twice); the node's children stay (it has none)"""
    tree.N[h][:] = 0
    tree.V[h][:] = 0.0
    tree.N[h][P] = prior_n
    tree.V[h][P] = prior_v
    tree.Nh[h] = int(tree.N[h].sum())


def search(o, states, belief, history, prev_ob, R, W, S, D, discount, ucb_c, seed, lane0, t0, trees=None, C=None, logn=None, P=0,
           prior_n=0, prior_v=0.0, nthreads=4, mutate=None):
    """pomdp_tree_search_preferred_resume -> tp.search's dict ("prior_sizes" aside) plus `trees` (the list after the search, to
    hand to tk.advance() or back in), `full` (int [R * W]: the simulations of each tree that met a full pool) and, in "stats",
    COUNTERS.  trees: a list of tk.KTree / None per tree, or None for all empty; the trees handed in are modified in place.
    C: the node capacity (default S + 1); logn: the table (default tp.log_table(S, A, prior_n), the anchor's)."""
    assert mutate is None or mutate in MUTATIONS
    n, A = R * W, o.n_actions
    rock = rr.is_rock(o)
    K = A - 5 if rock else 0
    C = S + 1 if C is None else C
    logn = tp.log_table(S, A, prior_n) if logn is None else logn
    assert len(logn) - 1 >= A * prior_n + 1
    if mutate == "nh_clamp_short":
        logn = logn[:-1]
    trees = [None] * n if trees is None else list(trees)
    kept = np.zeros(n, np.int64)                                         # nodes [0, kept[i]) were there before this search
    for i in range(n):
        if trees[i] is None:
            trees[i] = tk.KTree(A)
        else:
            kept[i] = len(trees[i].N)
        assert len(trees[i].N) <= C
    root_of = np.arange(n) // W
    ar = np.arange(n)
    sim_ret = np.zeros((S, n), np.float64)
    sim_steps = np.zeros((S, n), np.int32)
    sim_tree_steps = np.zeros((S, n), np.int32)
    full = np.zeros(n, np.int64)
    no_done = np.zeros(n, np.uint8)
    stats = {c: 0 for c in COUNTERS}
    root_prior_size = np.zeros(n, np.int64)
    ever_checked = np.zeros((max(K, 1), n), bool)
    hs_fields = ("size", "last_action", "last_ob") + (("total_sample", "total_move") if rock else ())
    for s in range(S):
        tsim = (t0 + s * D) & M64
        if P:
            x = ts.tree_words(seed, lane0, n, tsim)
            col = root_of * P + ((x * np.uint64(P)) >> np.uint64(32)).astype(np.int64)
            st = np.ascontiguousarray(states[:, col])
        else:
            st = np.ascontiguousarray(states[:, root_of])
        bel, hs, pob = rr.expand(o, belief, history, prev_ob, R, W)      # the private column of every tree, from its root
        if s == 0 and rock:
            stats["nan_prob"] += int(np.isnan(bel.prob_valuable).sum())
        stats["from_empty_history"] += int((hs.size == 0).sum())
        checked = np.zeros((max(K, 1), n), bool)
        repeated = np.zeros(n, bool)
        reused = np.zeros(n, bool)
        h = np.zeros(n, np.int64)
        k0 = np.full(n, -1, np.int64)
        words = [None] * n
        acc = np.zeros(n, np.float64)
        disc = np.ones(n, np.float64)
        paths = [[] for _ in range(n)]
        active = np.ones(n, bool)
        done = np.zeros(n, bool)
        fresh = np.zeros(n, bool)                                        # the step before created node h[i]
        forced = np.zeros(n, bool)                                       # a mutation's: the step before met a full pool
        for k in range(D):
            lists, lens = ol._batch_legal(o, st)
            plists, plens = ol._batch_preferred(o, st, hs, bel)
            rolling = k0 >= 0
            active &= ~done & (np.where(rolling, plens, lens) > 0)
            if not active.any():
                break
            # the policy's branches, on the list this step computed
            fb = np.zeros(n, bool)
            if rock:
                ck = rr.check_ok(bel)
                uncollected = rr.rock_codes(o, st) != 1
                fb = active & (lens == plens) & (lists == plists).all(axis=1) & (uncollected & ~ck).any(axis=0)
                stats["fallback"] += int(fb.sum())
                stats["sample_rule"] += int((active & (plens == 1) & (plists[:, 0] == 4)).sum())
                all_bad = ~(uncollected & (hs.total_move >= 0)).any(axis=0)
                stats["all_bad_east"] += int((active & all_bad & (plens == 1) & (plists[:, 0] == 1)).sum())
                mv0, sm0 = hs.total_move >= 0, hs.total_sample > 0
            if o.name == "tag":
                agent = (st[0] & np.uint32(31)).astype(np.int64)
                rule = active & (hs.size != 0) & (hs.last_ob == 29) & np.isin(agent, rr.TAG_CORNERS)
                assert not (rule & ~((plens == 1) & (plists[:, 0] == 4))).any()
                stats["corner_tag"] += int(rule.sum())
                stats["empty_history_all_five"] += int((active & (hs.size == 0) & (plens == 5)).sum())
            a = np.zeros(n, np.int32)
            for i in np.nonzero(active)[0]:
                t = trees[i]
                L = [int(v) for v in lists[i, :lens[i]]]
                Pl = [int(v) for v in plists[i, :plens[i]]]
                hi = int(h[i])
                # the new rule: node hi exists in the pool and the lane is about to choose at it
                at_node = k0[i] < 0 or fresh[i] or forced[i]
                if prior_n > 0 and at_node:
                    is_kept = hi < kept[i]
                    unprimed = t.Nh[hi] == 0 or forced[i] or (mutate == "reprime_kept_root" and is_kept and hi == 0 and s == 0 and k == 0)
                    if mutate == "never_prime_kept" and is_kept:
                        unprimed = False
                    if k0[i] < 0 and is_kept and t.Nh[hi] > 0:
                        reused[i] = True
                    if unprimed:                                         # P(h): the list this step's rollout pick would come from
                        stats["prior_from_fallback"] += int(fb[i])
                        stats["late_priors"] += int(is_kept)
                        set_priors(t, hi, Pl, prior_n, prior_v)
                        if hi == 0:
                            root_prior_size[i] = len(Pl)
                fresh[i] = forced[i] = False
                if k0[i] < 0:
                    a[i] = t.select(hi, L, ucb_c, logn)
                else:
                    a[i] = Pl[(int(words[i][k - int(k0[i])]) * len(Pl)) >> 32]
            if rock:
                chk = active & (a >= 5)
                j = np.where(chk, a - 5, 0)
                stats["fallback_check_of_closed"] += int((fb & chk & ~ck[j, ar]).sum())
                first = chk & ~checked[j, ar]
                stats["recheck_across_sims"] += int((first & ever_checked[j, ar]).sum())
                repeated |= chk & checked[j, ar]
                checked[j[chk], ar[chk]] = True
            nx = st.copy()
            ob, rew, dn, _ = o.batch_step(nx, a, seed, lane0, (tsim + k) & M64, auto_reset=False, done=no_done.copy(),
                                          nthreads=nthreads)
            for i in np.nonzero(active)[0]:
                st[:, i] = nx[:, i]
                done[i] = dn[i] != 0
                sim_steps[s, i] = k + 1
                r = np.float64(rew[i])
                if k0[i] < 0:
                    paths[i].append((int(h[i]), int(a[i]), r))
                    if not done[i]:
                        kids = trees[i].children[h[i]]
                        key = (int(a[i]), int(ob[i]))
                        if key in kids:
                            h[i] = kids[key]
                        else:
                            if len(trees[i].N) < C:
                                h[i] = kids[key] = trees[i].new_node()
                                fresh[i] = True
                            else:
                                full[i] += 1                             # no node, nothing primed; the rollout starts all the same
                                forced[i] = mutate == "prime_on_full_pool"
                            k0[i] = k + 1
                            words[i] = stream_words(seed, lane0 + i, (tsim + int(k0[i])) & M64, ts.STREAM_ROLLOUT,
                                                    max(D - int(k0[i]), 1))
                else:
                    acc[i] = acc[i] + disc[i] * r
                    disc[i] = disc[i] * np.float64(discount)
            # the private copies after the executed step, in the tree and in the rollout alike (tp.search)
            keep = np.nonzero(~active)[0]
            hs0 = {f: getattr(hs, f).copy() for f in hs_fields}
            act = np.where(active, a, 0).astype(np.int32)
            obs = np.where(active, ob, 0).astype(np.int32)
            dnn = np.where(active, dn, 1).astype(np.uint8)
            if rock:
                bel.update(st, act, obs, dnn, auto_reset=False)
            hs.append(pob, act, obs, dnn, auto_reset=False)
            for f in hs_fields:
                getattr(hs, f)[..., keep] = hs0[f][..., keep]
            pob = np.ascontiguousarray(np.where(active, ob, pob).astype(np.int32))
            if rock:
                ck2 = rr.check_ok(bel)
                stats["check_ok_cleared"] += int((ck & ~ck2).sum())
                stats["check_ok_set_again"] += int((~ck & ck2).sum())
                mv1, sm1 = hs.total_move >= 0, hs.total_sample > 0
                stats["move_bit_up"] += int((~mv0 & mv1).sum())
                stats["move_bit_down"] += int((mv0 & ~mv1).sum())
                stats["sample_bit_up"] += int((~sm0 & sm1).sum())
                stats["sample_bit_down"] += int((sm0 & ~sm1).sum())
        for i in range(n):
            sim_ret[s, i] = trees[i].backup(paths[i], acc[i], discount)
            sim_tree_steps[s, i] = len(paths[i])
        stats["repeat_check"] += int(repeated.sum())
        stats["kept_primed_reused"] += int(reused.sum())
        ever_checked |= checked
        if rock:
            stats["nan_prob"] += int(np.isnan(bel.prob_valuable).sum())
    tv = np.stack([t.N[0] for t in trees]).astype(np.int32)
    tq = np.stack([t.V[0] for t in trees]).astype(np.float64)
    out = ts.merge(tv, tq, R, W)
    out.update(tree_visits=tv, tree_q=tq, n_nodes=tk.n_nodes_of(trees), sim_ret=sim_ret, sim_steps=sim_steps,
               sim_tree_steps=sim_tree_steps, stats=stats, root_prior_size=root_prior_size, trees=trees, full=full)
    return out
