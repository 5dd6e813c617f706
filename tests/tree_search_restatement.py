"""CPU restatement of the tree-search contract (include/pomdp_hip.h: pomdp_tree_search), written from the header's words on top
of the oracle: every (simulation, step) is one OracleEnv.batch_step(auto_reset=False) over all R * W lanes, the legal lists are
ol._batch_legal's, the TREE and ROLLOUT words come from oracle.philox_ref, and a tree is a list of nodes with Python dicts for
the children.  Shared by test_tree_search_host.py and test_gpu_tree_search.py.

`mutate` exists for the host test's self-check only: each value breaks one rule of the contract by one token, and the host
test shows that its properties then fail (test_tree_search_host.py: test_every_rule_is_pinned_by_a_property)."""
import math

import numpy as np

from oracle import oracle_lib as ol
from oracle.philox_ref import philox4x32_10, stream_words

STREAM_ROLLOUT = 5
STREAM_TREE = 9
M64 = (1 << 64) - 1
MUTATIONS = ("unvisited_last", "last_maximum", "k0_at_root", "backup_from_root")


def log_table(S):
    """logn of the contract: logn[n] = log(n) on the host; entry 0 is never read"""
    return np.array([-np.inf] + [math.log(k) for k in range(1, S + 1)], np.float64)


def tree_words(seed, lane0, n, t):
    """x: word 0 of block 0 of stream TREE at (seed, lane0 + i, t), i < n"""
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = (lane0 + np.arange(n, dtype=np.uint64)) & 0xFFFFFFFF
    ctr[:, 1] = t & 0xFFFFFFFF
    ctr[:, 2] = (t >> 32) & 0xFFFFFFFF
    ctr[:, 3] = STREAM_TREE << 24
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, key)[:, 0].astype(np.uint64)


class Tree(object):
    def __init__(self, A):
        self.A = A
        self.N, self.V, self.children = [], [], []
        self.new_node()

    def new_node(self):
        self.N.append(np.zeros(self.A, np.int32))
        self.V.append(np.zeros(self.A, np.float64))
        self.children.append({})
        return len(self.N) - 1

    def select(self, h, L, c, logn, mutate):
        N, V = self.N[h], self.V[h]
        fresh = [a for a in L if N[a] == 0]
        if fresh:
            return fresh[-1] if mutate == "unvisited_last" else fresh[0]
        ln = logn[int(N.sum())]
        best, bu = None, None
        for a in L:
            ratio = ln / np.float64(N[a])
            bonus = np.float64(c) * np.sqrt(ratio)
            u = V[a] + bonus
            if best is None or (u >= bu if mutate == "last_maximum" else u > bu):
                best, bu = a, u
        return best

    def backup(self, path, acc, discount, mutate):
        rt = np.float64(acc)
        for h, a, r in (path if mutate == "backup_from_root" else reversed(path)):
            rt = np.float64(r) + np.float64(discount) * rt
            self.N[h][a] += 1
            self.V[h][a] = self.V[h][a] + (rt - self.V[h][a]) / np.float64(self.N[h][a])
        return rt


def merge(tree_visits, tree_q, R, W):
    """the per-root merge -> dict(q, visits, best, value)"""
    A = tree_visits.shape[1]
    out = dict(q=np.zeros((R, A), np.float64), visits=np.zeros((R, A), np.int32), best=np.full(R, -1, np.int32),
               value=np.zeros(R, np.float64))
    for r in range(R):
        for a in range(A):
            total, visits = np.float64(0.0), 0
            for w in range(W):
                n = tree_visits[r * W + w, a]
                total = total + np.float64(n) * tree_q[r * W + w, a]
                visits += int(n)
            out["visits"][r, a] = visits
            out["q"][r, a] = total / np.float64(visits) if visits > 0 else 0.0
        b = -1
        for a in range(A):
            if out["visits"][r, a] > 0 and (b < 0 or out["q"][r, a] > out["q"][r, b]):
                b = a
        out["best"][r] = b
        out["value"][r] = out["q"][r, b] if b >= 0 else 0.0
    return out


def search(o, roots, R, W, S, D, discount, ucb_c, seed, lane0, t0, particles=None, P=0, nthreads=4, mutate=None):
    """pomdp_tree_search -> dict(q, visits, best, value, tree_visits, tree_q, n_nodes, sim_ret, sim_steps, sim_tree_steps).
    roots: uint32 [words, R] (true states) or, with particles (uint32 [words, R * P]), unused."""
    assert mutate is None or mutate in MUTATIONS
    n, A = R * W, o.n_actions
    logn = log_table(S)
    trees = [Tree(A) for _ in range(n)]
    root_of = np.arange(n) // W
    sim_ret = np.zeros((S, n), np.float64)
    sim_steps = np.zeros((S, n), np.int32)
    sim_tree_steps = np.zeros((S, n), np.int32)
    no_done = np.zeros(n, np.uint8)
    for s in range(S):
        ts = (t0 + s * D) & M64
        if particles is not None:
            x = tree_words(seed, lane0, n, ts)
            col = root_of * P + ((x * np.uint64(P)) >> np.uint64(32)).astype(np.int64)
            st = np.ascontiguousarray(particles[:, col])
        else:
            st = np.ascontiguousarray(roots[:, root_of])
        h = np.zeros(n, np.int64)
        k0 = np.full(n, -1, np.int64)
        words = [None] * n
        acc = np.zeros(n, np.float64)
        disc = np.ones(n, np.float64)
        paths = [[] for _ in range(n)]
        active = np.ones(n, bool)
        done = np.zeros(n, bool)
        for k in range(D):
            lists, lens = ol._batch_legal(o, st)
            active &= ~done & (lens > 0)
            if not active.any():
                break
            a = np.zeros(n, np.int32)
            for i in np.nonzero(active)[0]:
                L = [int(v) for v in lists[i, :lens[i]]]
                if k0[i] < 0:
                    a[i] = trees[i].select(h[i], L, ucb_c, logn, mutate)
                else:
                    a[i] = L[(int(words[i][k - int(k0[i])]) * len(L)) >> 32]
            nx = st.copy()
            ob, rew, dn, _ = o.batch_step(nx, a, seed, lane0, (ts + k) & M64, auto_reset=False, done=no_done.copy(),
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
                            tk = ts if mutate == "k0_at_root" else (ts + int(k0[i])) & M64
                            words[i] = stream_words(seed, lane0 + i, tk, STREAM_ROLLOUT, max(D - int(k0[i]), 1))
                else:
                    acc[i] = acc[i] + disc[i] * r
                    disc[i] = disc[i] * np.float64(discount)
        for i in range(n):
            sim_ret[s, i] = trees[i].backup(paths[i], acc[i], discount, mutate)
            sim_tree_steps[s, i] = len(paths[i])
    tv = np.stack([t.N[0] for t in trees]).astype(np.int32)
    tq = np.stack([t.V[0] for t in trees]).astype(np.float64)
    out = merge(tv, tq, R, W)
    out.update(tree_visits=tv, tree_q=tq, n_nodes=np.array([len(t.N) for t in trees], np.int32), sim_ret=sim_ret,
               sim_steps=sim_steps, sim_tree_steps=sim_tree_steps)
    return out
