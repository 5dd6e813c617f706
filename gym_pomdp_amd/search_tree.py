"""The search trees of BatchedEnv.search(tree=...) kept between real steps (include/pomdp_hip.h: pomdp_tree_search_resume,
pomdp_tree_search_preferred_resume, pomdp_tree_advance): the device-resident node pools, and the step that makes the real
step's child the new root."""
import ctypes as C
import math

import numpy as np
import torch

from . import _native


class SearchTree(object):
    """W = trees_per_root trees per lane of `env`, each a pool of C = node_capacity nodes for searches of depth D, empty at
    first.  env.search(..., tree=tree) resumes every tree from the nodes it holds; advance(action, ob, drop=None) keeps, per
    tree, the subtree under the root's child (action[r], ob[r]) and makes it the new root — a tree without that child, with
    an action outside [0, A) (a search's best == -1) or with drop[r] != 0 becomes empty.  env.search_step(..., tree=tree) does
    both around the real step.  Two workspaces are used in turn (the copy goes from one to the other), so a call allocates
    nothing on the device except when the log table grows.

    A node's visit count Nh grows by at most sims_per_tree per search and indexes the search's log table, so the tree counts
    its searches since the last full clear() and keeps a table of at least searches * S + 1 entries, grown geometrically.
    Merged visit counts are int32: once W * searches * S would pass 2^31 - 1 the next search raises ValueError — clear() the
    tree (it restarts the count).

    A tree is bound to the policy it is grown under.  policy="uniform" (the default) is resumed by the uniform search.
    policy="preferred" on an env with a preferred-action policy of its own (RockSample with use_heuristic=True, Tag) is
    resumed by search(policy="preferred", history=...) and carries the node priors prior_n / prior_v: a tree grown without
    priors must not be continued by a search that assumes them, nor the other way round.  Priors are laid once per node, so
    Nh can reach searches * S + A * prior_n, and the table and the int32 bound count that term.  On the other envs the
    preferred search IS the uniform one: policy="preferred" with prior_n == 0 gives a uniform tree, prior_n > 0 raises.

    n_nodes: int32 [R * W], the nodes each tree holds (< 1: empty).  to_host(i): tree i decoded, for tests and debugging."""

    def __init__(self, env, trees_per_root, node_capacity=None, depth=64, sims_per_tree=None, policy="uniform", prior_n=0,
                 prior_v=0.0):
        W, D = int(trees_per_root), int(depth)
        if policy not in ("uniform", "preferred"):
            raise ValueError("search_tree: policy must be 'uniform' or 'preferred', got %r" % (policy,))
        prior_n, prior_v = int(prior_n), float(prior_v)
        if prior_n < 0 or prior_n > 65535 or not math.isfinite(prior_v):
            raise ValueError("search_tree: needs 0 <= prior_n <= 65535 and a finite prior_v, got %r, %r" % (prior_n, prior_v))
        own_policy = env.env_name == "tag" or (env.env_name == "rock" and env._use_heuristic)
        if prior_n > 0 and not (policy == "preferred" and own_policy):
            raise ValueError("search_tree: prior_n > 0 needs policy='preferred' on an env with a preferred-action policy of its "
                             "own (RockSample with use_heuristic=True, Tag): a uniform prior over the legal list steers nothing")
        self.policy = "preferred" if (policy == "preferred" and own_policy) else "uniform"
        self.prior_n, self.prior_v = (prior_n, prior_v) if self.policy == "preferred" else (0, 0.0)
        if node_capacity is None:
            if sims_per_tree is None:
                raise ValueError("search_tree: give node_capacity, or sims_per_tree= for the default 2 * sims_per_tree + 1")
            node_capacity = 2 * int(sims_per_tree) + 1
        Cn = int(node_capacity)
        R = env.batch_size
        if W < 1 or Cn < 1 or D < 0 or env.lane_offset * W + R * W > 1 << 32:
            raise ValueError("search_tree: needs trees_per_root >= 1, node_capacity >= 1, depth >= 0 and the trees' global lanes "
                             "in [0, 2^32)")
        self.env = env
        self.trees_per_root, self.node_capacity, self.depth = W, Cn, D
        self.n_roots, self.n_actions = R, env.action_space.n
        self.device = env.device
        self._kind = _native.ENV_KIND[env.env_name]
        self._lib = _native.lib()
        n = R * W
        self._bytes = int(self._lib.pomdp_tree_keep_workspace(self._kind, env._params_ref, n, Cn, D))
        if self._bytes == 0 and n > 0:
            raise ValueError("search_tree: pomdp_tree_keep_workspace refuses %d trees x %d nodes x depth %d" % (n, Cn, D))
        self._ws = [torch.empty((self._bytes // 16, 2), dtype=torch.float64, device=self.device) for _ in range(2)]   # 16-byte units
        self._counts = [torch.zeros(n, dtype=torch.int32, device=self.device) for _ in range(2)]
        self._cur = 0
        self.searches = 0
        self._logn = None
        self._policy_workspace = None                        # RockSample's scratch of the preferred search, held for reuse

    @property
    def n_nodes(self):
        """int32 [R * W] (the live buffer: the next advance() writes the other one)"""
        return self._counts[self._cur]

    def _belongs(self, env, W, D):
        e = self.env
        return (env.env_name == e.env_name and env.batch_size == self.n_roots and env.lane_offset == e.lane_offset
                and bytes(env._params) == bytes(e._params) and int(W) == self.trees_per_root and int(D) == self.depth)

    def _keep(self, which, logn_len):
        return _native.PlanTreeKeep(workspace=self._ws[which].data_ptr() if self._bytes else None, workspace_bytes=self._bytes,
                                    n_nodes=self._counts[which].data_ptr(), node_capacity=self.node_capacity, logn_len=logn_len)

    def _begin_search(self, S):
        """-> (the log table, the pomdp_tree_keep of the live trees) for one more search of S simulations per tree"""
        need = (self.searches + 1) * int(S) + self.n_actions * self.prior_n   # the largest Nh the search can reach
        if self.trees_per_root * need > 0x7FFFFFFF:
            raise ValueError("search: trees_per_root * (searches * sims_per_tree + n_actions * prior_n) would pass 2^31 - 1 "
                             "(merged visit counts are int32) after %d searches: clear() the SearchTree" % self.searches)
        if self._logn is None or self._logn.numel() < need + 1:
            n_log = min(max(need + 1, 2 * (0 if self._logn is None else self._logn.numel())), 0x7FFFFFFF // self.trees_per_root + 1)
            table = np.empty(n_log, np.float64)
            table[0] = -np.inf
            table[1:] = [math.log(k) for k in range(1, n_log)]
            self._logn = torch.from_numpy(table).to(self.device)
        self.searches += 1
        return self._logn, self._keep(self._cur, self._logn.numel())

    def advance(self, action, ob, drop=None):
        """pomdp_tree_advance: every tree of lane r keeps the subtree under (action[r], ob[r]) — or nothing, where there is no
        such child, the action is outside [0, A) or drop[r] != 0 — and the workspaces swap.  Asynchronous."""
        at, ot = self._col(action, torch.int32, "action"), self._col(ob, torch.int32, "ob")
        dt = None if drop is None else self._col(drop, torch.uint8, "drop")
        src, dst = self._keep(self._cur, 2), self._keep(1 - self._cur, 2)
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_tree_advance(self._kind, self.env._params_ref, self.n_roots, self.trees_per_root, self.depth,
                                              C.byref(src), C.byref(dst), at.data_ptr(), ot.data_ptr(),
                                              None if dt is None else dt.data_ptr(), self.env._stream())
            _native.check(rc, "pomdp_tree_advance")
        self._cur = 1 - self._cur

    def clear(self, where=None):
        """Empty every tree (and restart the count of searches), or the trees of the lanes with where[r] != 0."""
        if where is None:
            self.n_nodes.zero_()
            self.searches = 0
            return
        m = self._col(where, torch.uint8, "where").bool()
        self.n_nodes.view(self.n_roots, self.trees_per_root)[m] = 0

    def _col(self, x, dtype, what):
        t = x.to(self.device) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), device=self.device)
        t = t.reshape(-1)
        if t.shape != (self.n_roots,):
            raise ValueError("%s must have shape (%d,), got %s" % (what, self.n_roots, tuple(t.shape)))
        if dtype == torch.uint8:
            t = t != 0
        return t.to(dtype).contiguous()

    def to_host(self, i):
        """Tree i decoded from the workspace: {path: (N int32 [A], V float64 [A], Nh)}, path = the tuple of (action,
        observation) pairs from the root — () is the root; {} for an empty tree.  Synchronises."""
        A, Cn = self.n_actions, self.node_capacity
        n = min(int(self.n_nodes[i].item()), Cn)
        if n < 1:
            return {}
        per = self._bytes // (self.n_roots * self.trees_per_root)
        raw = self._ws[self._cur].reshape(-1)[i * per // 8:(i + 1) * per // 8].cpu().numpy().view(np.uint8)
        edge = raw[:16 * Cn * A].view(np.dtype([("v", "<f8"), ("n", "<i4"), ("child", "<i4")])).reshape(Cn, A)
        node = raw[16 * Cn * A:16 * Cn * (A + 1)].view(np.int32).reshape(Cn, 4)       # ob, next sibling, Nh, spare
        res, todo = {}, [(0, ())]
        while todo:
            h, path = todo.pop()
            if path in res or len(res) >= n:
                raise RuntimeError("to_host: tree %d is malformed at node %d" % (i, h))
            res[path] = (edge["n"][h].copy(), edge["v"][h].copy(), int(node[h, 2]))
            for a in range(A):
                c, seen = int(edge["child"][h, a]), 0
                while c:
                    if not 0 < c < n or seen >= n:
                        raise RuntimeError("to_host: tree %d has a bad child link at node %d" % (i, h))
                    todo.append((c, path + ((a, int(node[c, 0])),)))
                    c, seen = int(node[c, 1]), seen + 1
        return res
