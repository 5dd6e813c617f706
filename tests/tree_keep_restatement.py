"""CPU restatement of the kept-tree contract (include/pomdp_hip.h: pomdp_tree_search_resume, pomdp_tree_advance) on top of
tree_search_restatement (imported unchanged): a search that takes initial trees, a node capacity C and a log table, the advance
to the subtree under the real step, and the canonical form SearchTree.to_host returns.  A tree is a KTree — ts.Tree plus the
stored visit count Nh per node — and None stands for an empty tree (n_nodes 0).  Shared by test_tree_keep_host.py and
test_gpu_tree_keep.py.

`mutate` exists for the host test's self-check only: each value breaks one of the NEW rules by one token
(test_tree_keep_host.py: test_every_new_rule_is_pinned_by_a_property)."""
import numpy as np

import tree_search_restatement as ts
from oracle import oracle_lib as ol
from oracle.philox_ref import stream_words

M64 = ts.M64
MUTATIONS = ("no_match_keeps_root", "drop_ignored", "full_pool_creates", "nh_not_carried")


class KTree(ts.Tree):
    def __init__(self, A):
        self.Nh = []
        ts.Tree.__init__(self, A)

    def new_node(self):
        self.Nh.append(0)
        return ts.Tree.new_node(self)

    def select(self, h, L, c, logn):
        """step 2 with the stored Nh, clamped to the table's last entry"""
        N, V = self.N[h], self.V[h]
        fresh = [a for a in L if N[a] == 0]
        if fresh:
            return fresh[0]
        ln = logn[min(max(self.Nh[h], 0), len(logn) - 1)]
        best, bu = None, None
        with np.errstate(invalid="ignore"):                                # Nh == 0 under a mutation: sqrt(-inf), as the device computes it
            for a in L:
                ratio = ln / np.float64(N[a])
                bonus = np.float64(c) * np.sqrt(ratio)
                u = V[a] + bonus
                if best is None or u > bu:
                    best, bu = a, u
        return best

    def backup(self, path, acc, discount):
        rt = np.float64(acc)
        for h, a, r in reversed(path):
            rt = np.float64(r) + np.float64(discount) * rt
            self.N[h][a] += 1
            self.V[h][a] = self.V[h][a] + (rt - self.V[h][a]) / np.float64(self.N[h][a])
            self.Nh[h] += 1
        return rt


def canon(tree):
    """{path: (N row, V row, Nh)}, path = the tuple of (action, observation) pairs from the root; {} for an empty tree"""
    if tree is None:
        return {}
    res, todo = {}, [(0, ())]
    while todo:
        h, path = todo.pop()
        res[path] = (tree.N[h].copy(), tree.V[h].copy(), int(tree.Nh[h]))
        for (a, ob), c in tree.children[h].items():
            todo.append((c, path + ((a, ob),)))
    return res


def same_canon(x, y):
    """bit for bit"""
    if set(x) != set(y):
        return False
    for k in x:
        (n1, v1, h1), (n2, v2, h2) = x[k], y[k]
        if h1 != h2 or not np.array_equal(np.asarray(n1, np.int32), np.asarray(n2, np.int32)):
            return False
        if not np.array_equal(np.ascontiguousarray(v1, np.float64).view(np.uint64), np.ascontiguousarray(v2, np.float64).view(np.uint64)):
            return False
    return True


def n_nodes_of(trees):
    return np.array([0 if t is None else len(t.N) for t in trees], np.int32)


def advance(trees, W, action, ob, drop=None, mutate=None):
    """pomdp_tree_advance -> the new list of trees (None: empty).  The copy is breadth-first; its numbering is not part of
    what canon() or the node count show, so the children of one (h, a) are taken in the dict's order."""
    assert mutate is None or mutate in MUTATIONS
    out = []
    for i, t in enumerate(trees):
        r = i // W
        a, o = int(action[r]), int(ob[r])
        if drop is not None and drop[r] and mutate != "drop_ignored":
            out.append(None)
            continue
        if t is None or a < 0 or a >= t.A:
            out.append(None)
            continue
        c = t.children[0].get((a, o))
        if c is None:
            out.append(t if mutate == "no_match_keeps_root" else None)
            continue
        nt = KTree(t.A)                                                    # the queue grows while it is scanned
        queue, q = [c], 0
        while q < len(queue):
            s = queue[q]
            nt.N[q] = t.N[s].copy()
            nt.V[q] = t.V[s].copy()
            nt.Nh[q] = 0 if (mutate == "nh_not_carried" and q == 0) else t.Nh[s]
            for key in sorted(t.children[s], key=lambda k: k[0]):          # ascending action; one (h, a)'s children in dict order
                idx = nt.new_node()
                assert idx == len(queue)
                queue.append(t.children[s][key])
                nt.children[q][key] = idx
            q += 1
        out.append(nt)
    return out


def search(o, roots, R, W, S, D, discount, ucb_c, seed, lane0, t0, trees=None, C=None, logn=None, particles=None, P=0, nthreads=4,
           mutate=None):
    """pomdp_tree_search_resume -> ts.search's dict plus `trees` (the list after the search, to hand to advance() or back in)
    and `full` (int [R * W]: the simulations of each tree that met a full pool).  trees: a list of KTree / None per tree, or
    None for all empty; the trees handed in are modified in place.  C: the node capacity (default S + 1); logn: the table
    (default ts.log_table(S))."""
    assert mutate is None or mutate in MUTATIONS
    n, A = R * W, o.n_actions
    C = S + 1 if C is None else C
    logn = ts.log_table(S) if logn is None else logn
    trees = [None] * n if trees is None else list(trees)
    for i in range(n):
        if trees[i] is None:
            trees[i] = KTree(A)
        assert len(trees[i].N) <= C
    root_of = np.arange(n) // W
    sim_ret = np.zeros((S, n), np.float64)
    sim_steps = np.zeros((S, n), np.int32)
    sim_tree_steps = np.zeros((S, n), np.int32)
    full = np.zeros(n, np.int64)
    no_done = np.zeros(n, np.uint8)
    for s in range(S):
        tsim = (t0 + s * D) & M64
        if particles is not None:
            x = ts.tree_words(seed, lane0, n, tsim)
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
                    a[i] = trees[i].select(h[i], L, ucb_c, logn)
                else:
                    a[i] = L[(int(words[i][k - int(k0[i])]) * len(L)) >> 32]
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
                            if len(trees[i].N) < C or mutate == "full_pool_creates":
                                h[i] = kids[key] = trees[i].new_node()
                            else:
                                full[i] += 1                                   # no node; the rollout starts all the same
                            k0[i] = k + 1
                            words[i] = stream_words(seed, lane0 + i, (tsim + int(k0[i])) & M64, ts.STREAM_ROLLOUT, max(D - int(k0[i]), 1))
                else:
                    acc[i] = acc[i] + disc[i] * r
                    disc[i] = disc[i] * np.float64(discount)
        for i in range(n):
            sim_ret[s, i] = trees[i].backup(paths[i], acc[i], discount)
            sim_tree_steps[s, i] = len(paths[i])
    tv = np.stack([t.N[0] for t in trees]).astype(np.int32)
    tq = np.stack([t.V[0] for t in trees]).astype(np.float64)
    out = ts.merge(tv, tq, R, W)
    out.update(tree_visits=tv, tree_q=tq, n_nodes=n_nodes_of(trees), sim_ret=sim_ret, sim_steps=sim_steps,
               sim_tree_steps=sim_tree_steps, trees=trees, full=full)
    return out
