"""CPU restatement of the preferred-policy tree search (include/pomdp_hip.h: pomdp_tree_search_preferred), written from the
header's words on top of the oracle: tree_search_restatement's loop, trees and merge, with one PRIVATE column of policy inputs
per tree (preferred_rollout_restatement.expand), refilled from the roots at every simulation; the lists come from
ol._batch_preferred (which holds the fallback to the legal list), the updates from Belief.update / HistorySums.append(
auto_reset=False).  Shared by test_tree_search_preferred_host.py and test_gpu_tree_search_preferred.py.

search() also counts, over live simulation-steps, preferred_rollout_restatement's COUNTERS (on the list every step computes,
whether the step picked from it or not) and two of its own:
  recheck_across_sims   a simulation's first CHECK of rock j in a tree where an EARLIER simulation CHECKed j (it must read the
                        root's entry, not the slot the earlier simulation left)
  prior_from_fallback   nodes whose P(h) was the legal fallback (prior_n > 0 only)

`mutate` exists for the host test's self-check only: each value breaks one rule by one token, and the host test shows that the
rule's property then fails."""
import numpy as np

import preferred_rollout_restatement as rr
import tree_search_restatement as ts
from oracle import oracle_lib as ol
from oracle.philox_ref import stream_words

M64 = ts.M64
MUTATIONS = ("no_refill", "no_tree_update", "no_fallback_priors", "root_priors_every_sim", "nh_without_priors")
KEY_MUTATIONS = ("k0_at_root",)          # tree_search_restatement's, for test_tree_edges_host.py: the ROLLOUT counter t_s, not t_s + k0
COUNTERS = rr.COUNTERS + ("recheck_across_sims", "prior_from_fallback")


def log_table(S, A, prior_n):
    """logn of the contract: S + 1 + A * prior_n entries, logn[n] = log(n) on the host"""
    return ts.log_table(S + A * prior_n)


class PriorTree(ts.Tree):
    """ts.Tree with priors: N and V of a node's preferred actions start at (prior_n, prior_v); Nh = sum_a N(h,a) counts them"""

    def __init__(self, A):
        self.prior_total = []
        ts.Tree.__init__(self, A)

    def new_node(self):
        self.prior_total.append(0)
        return ts.Tree.new_node(self)

    def set_priors(self, h, P, prior_n, prior_v):
        self.N[h][:] = 0
        self.V[h][:] = 0.0
        self.N[h][P] = prior_n
        self.V[h][P] = prior_v
        self.prior_total[h] = prior_n * len(P)

    def select(self, h, L, c, logn, mutate):
        N, V = self.N[h], self.V[h]
        fresh = [a for a in L if N[a] == 0]
        if fresh:
            return fresh[0]
        nh = int(N.sum()) - (self.prior_total[h] if mutate == "nh_without_priors" else 0)
        ln = logn[nh]
        best, bu = None, None
        with np.errstate(invalid="ignore", divide="ignore"):
            for a in L:
                ratio = ln / np.float64(N[a])
                bonus = np.float64(c) * np.sqrt(ratio)
                u = V[a] + bonus
                if best is None or u > bu:
                    best, bu = a, u
        return best


def search(o, states, belief, history, prev_ob, R, W, S, D, discount, ucb_c, seed, lane0, t0, P=0, prior_n=0, prior_v=0.0,
           nthreads=4, mutate=None):
    """pomdp_tree_search_preferred -> ts.search's dict plus "stats" (COUNTERS), "root_prior_size" int [R * W] (|P(0)|, 0
    without priors) and "prior_sizes": per tree, |P(h)| of every node that got priors.
    states: uint32 [words, R] (P == 0: the true states) or [words, R * P]; belief / history / prev_ob: the roots' policy inputs
    as preferred_rollout_restatement takes them."""
    assert mutate is None or mutate in MUTATIONS + KEY_MUTATIONS
    n, A = R * W, o.n_actions
    rock = rr.is_rock(o)
    K = A - 5 if rock else 0
    logn = log_table(S, A, prior_n)
    trees = [PriorTree(A) for _ in range(n)]
    root_of = np.arange(n) // W
    ar = np.arange(n)
    sim_ret = np.zeros((S, n), np.float64)
    sim_steps = np.zeros((S, n), np.int32)
    sim_tree_steps = np.zeros((S, n), np.int32)
    no_done = np.zeros(n, np.uint8)
    stats = {c: 0 for c in COUNTERS}
    root_prior_size = np.zeros(n, np.int64)
    prior_sizes = [[] for _ in range(n)]
    ever_checked = np.zeros((max(K, 1), n), bool)
    hs_fields = ("size", "last_action", "last_ob") + (("total_sample", "total_move") if rock else ())
    bel = hs = pob = None
    for s in range(S):
        tsim = (t0 + s * D) & M64
        if P:
            x = ts.tree_words(seed, lane0, n, tsim)
            col = root_of * P + ((x * np.uint64(P)) >> np.uint64(32)).astype(np.int64)
            st = np.ascontiguousarray(states[:, col])
        else:
            st = np.ascontiguousarray(states[:, root_of])
        if s == 0 or mutate != "no_refill":                              # the private column of every tree, from its root
            bel, hs, pob = rr.expand(o, belief, history, prev_ob, R, W)
        if s == 0 and rock:
            stats["nan_prob"] += int(np.isnan(bel.prob_valuable).sum())
        stats["from_empty_history"] += int((hs.size == 0).sum())
        checked = np.zeros((max(K, 1), n), bool)
        repeated = np.zeros(n, bool)
        h = np.zeros(n, np.int64)
        k0 = np.full(n, -1, np.int64)
        words = [None] * n
        acc = np.zeros(n, np.float64)
        disc = np.ones(n, np.float64)
        paths = [[] for _ in range(n)]
        active = np.ones(n, bool)
        done = np.zeros(n, bool)
        unprimed = np.full(n, prior_n > 0 and (s == 0 or mutate == "root_priors_every_sim"))
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
                L = [int(v) for v in lists[i, :lens[i]]]
                Pl = [int(v) for v in plists[i, :plens[i]]]
                if unprimed[i]:                                          # P(h): the list this step's rollout pick would come from
                    unprimed[i] = False
                    stats["prior_from_fallback"] += int(fb[i])
                    if mutate == "no_fallback_priors" and fb[i]:
                        Pl_prior = []
                    else:
                        Pl_prior = Pl
                    trees[i].set_priors(h[i], Pl_prior, prior_n, prior_v)
                    prior_sizes[i].append(len(Pl_prior))
                    if h[i] == 0:
                        root_prior_size[i] = len(Pl_prior)
                if k0[i] < 0:
                    a[i] = trees[i].select(h[i], L, ucb_c, logn, mutate)
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
            in_tree = active & (k0 < 0)
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
                            h[i] = kids[key] = trees[i].new_node()
                            k0[i] = k + 1
                            unprimed[i] = prior_n > 0
                            tk = tsim if mutate == "k0_at_root" else (tsim + int(k0[i])) & M64
                            words[i] = stream_words(seed, lane0 + i, tk, ts.STREAM_ROLLOUT, max(D - int(k0[i]), 1))
                else:
                    acc[i] = acc[i] + disc[i] * r
                    disc[i] = disc[i] * np.float64(discount)
            # the private copies after the executed step, in the tree and in the rollout alike: one non-auto-reset step of
            # pomdp_heuristic_steps on live lanes; the others are marked done with a non-CHECK action and put back
            upd = active & ~in_tree if mutate == "no_tree_update" else active
            keep = np.nonzero(~upd)[0]
            hs0 = {f: getattr(hs, f).copy() for f in hs_fields}
            act = np.where(upd, a, 0).astype(np.int32)
            obs = np.where(upd, ob, 0).astype(np.int32)
            dnn = np.where(upd, dn, 1).astype(np.uint8)
            if rock:
                bel.update(st, act, obs, dnn, auto_reset=False)
            hs.append(pob, act, obs, dnn, auto_reset=False)
            for f in hs_fields:
                getattr(hs, f)[..., keep] = hs0[f][..., keep]
            pob = np.ascontiguousarray(np.where(upd, ob, pob).astype(np.int32))
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
            sim_ret[s, i] = trees[i].backup(paths[i], acc[i], discount, None)
            sim_tree_steps[s, i] = len(paths[i])
        stats["repeat_check"] += int(repeated.sum())
        ever_checked |= checked
        if rock:
            stats["nan_prob"] += int(np.isnan(bel.prob_valuable).sum())
    tv = np.stack([t.N[0] for t in trees]).astype(np.int32)
    tq = np.stack([t.V[0] for t in trees]).astype(np.float64)
    out = ts.merge(tv, tq, R, W)
    out.update(tree_visits=tv, tree_q=tq, n_nodes=np.array([len(t.N) for t in trees], np.int32), sim_ret=sim_ret,
               sim_steps=sim_steps, sim_tree_steps=sim_tree_steps, stats=stats, root_prior_size=root_prior_size,
               prior_sizes=prior_sizes)
    return out
