"""Controller — a finite-state controller for a batched env: K nodes, an action per node, a successor node per (node,
observation).  `env.run_controller(ctrl, steps)` plays the batch's episodes under it inside one fused loop on the device
(include/pomdp_hip.h: pomdp_controller_episodes): lane i takes action[node[i]], observes, moves to next[node[i]][ob].  A
memoryless ob -> action table, an open-loop plan, "listen twice, then open the other door" and whatever finite-memory policy a
search or a distilled network produces are all of this form; several controllers side by side (concat) are one controller, so a
population is evaluated in one call."""
import numpy as np
import torch

MAX_NODES = 4096          # include/pomdp_hip.h: pomdp_controller
MAX_EDGES = 16384         # n_nodes * n_obs


def _int_array(x, what):
    """an integer array-like (tensor, array, list) as an int64 numpy array"""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype.kind not in "iu":
        raise ValueError("Controller: %s must hold integers, got dtype %s" % (what, a.dtype))
    return a.astype(np.int64)


def _first_outside(a, hi):
    """index (a tuple) of the first entry of `a` outside [0, hi), or None"""
    bad = np.argwhere((a < 0) | (a >= hi))
    return tuple(int(v) for v in bad[0]) if len(bad) else None


def _as_int32(a):
    """int64 -> int32 without wrapping: a value outside int32 becomes -1 (invalid wherever it is used)"""
    return np.where((a < -(1 << 31)) | (a >= 1 << 31), -1, a).astype(np.int32)


class _LaneNodes(object):
    """What every controller class keeps per lane: `node` (int32 [N] on the env's device, lane i's current node; in/out of
    every run_controller call), the `start` nodes in their three forms, and reset_nodes().  A subclass sets env, device,
    n_nodes, n_obs and validate, then calls _init_nodes(start)."""

    def _init_nodes(self, start):
        self.node = torch.zeros(self.env.batch_size, dtype=torch.int32, device=self.device)
        self.start = start
        if self._start_kind != "table":
            self.reset_nodes()

    # ---- start nodes ---------------------------------------------------------------------------------------------------------
    @property
    def start(self):
        return self._start

    @start.setter
    def start(self, start):
        N = self.node.shape[0]
        if isinstance(start, (int, np.integer)):
            s, kind = np.asarray(int(start), np.int64), "int"
        else:
            s = _int_array(start, "start")
            kind = "lanes" if s.shape == (N,) else "table" if s.shape == (self.n_obs,) else None
            if kind is None:
                raise ValueError("%s: start must be an int, an int [%d] array (per lane) or an int [%d] table (per reset "
                                 "observation), got shape %s" % (type(self).__name__, N, self.n_obs, s.shape))
        if self.validate:
            bad = _first_outside(s.reshape(-1), self.n_nodes)
            if bad is not None:
                raise ValueError("%s: start%s = %d is outside [0, %d)"
                                 % (type(self).__name__, "" if kind == "int" else "[%d]" % bad[0], s.reshape(-1)[bad], self.n_nodes))
        self._start_kind = kind
        self._start = int(s) if kind == "int" else torch.as_tensor(_as_int32(s), device=self.device)

    def reset_nodes(self, ob=None, where=None):
        """Put lanes back on their start nodes: all of them, or those with where[i] != 0 (bool / integer [N]) — the companion
        of env.reset(where=env.done).  env.done is the live flag buffer and that reset clears it, so reset the nodes first, or
        keep the mask: `fin = env.done.clone(); ob = env.reset(where=fin); ctrl.reset_nodes(ob=ob, where=fin)`.  `ob` (int
        [N], what that reset returned) is needed when `start` is a table per reset observation; the entries of lanes outside
        `where` (-1 from a masked reset) are not used.  Plain torch, asynchronous.  Returns `node`."""
        N = self.node.shape[0]
        if self._start_kind == "int":
            new = torch.full_like(self.node, self._start)
        elif self._start_kind == "lanes":
            new = self._start
        else:
            if ob is None:
                raise ValueError("%s.reset_nodes: start is a table per reset observation — pass ob" % type(self).__name__)
            o = ob.to(self.device) if isinstance(ob, torch.Tensor) else torch.as_tensor(np.asarray(ob), device=self.device)
            if o.shape != (N,) or o.dtype.is_floating_point:
                raise ValueError("%s.reset_nodes: ob must be an int [%d] array" % (type(self).__name__, N))
            new = self._start[o.long().clamp(0, self.n_obs - 1)]
        if where is None:
            self.node.copy_(new)
        else:
            w = where.to(self.device) if isinstance(where, torch.Tensor) else torch.as_tensor(np.asarray(where), device=self.device)
            if w.shape != (N,) or w.dtype.is_floating_point:
                raise ValueError("%s.reset_nodes: where must be a bool / integer [%d] array" % (type(self).__name__, N))
            self.node.copy_(torch.where(w != 0, new, self.node))
        return self.node


class Controller(_LaneNodes):
    """Controller(env, action, next, start=0, validate=True)

    action: integer array-like [K] — the action of node q.  next: integer array-like [K, env.observation_space.n] — the
    successor of node q on observation o.  1 <= K <= 4096 and K * n_obs <= 16384 (the tables live in the workgroup's LDS).
    Checked on the host at construction: the shapes and limits, every action in [0, n_actions), every successor in [0, K);
    validate=False skips the range checks (the kernel then treats such an entry as the header says: a lane that meets it is
    left untouched, or keeps its node, and is counted in env.invalid_action_count()).

    start: where reset_nodes() puts a lane — an int, an int [N] array (per-lane start nodes; N = env.batch_size), or an int
    [n_obs] table indexed by the lane's reset observation (reset_nodes then needs `ob`).  An array of N entries is read as
    per-lane even where N == n_obs.

    `action`, `next` (int32, on the env's device) and `node` (int32 [N], lane i's current node; in/out of every run_controller
    call) are the tensors the kernel reads.  A new controller's lanes stand on their start nodes unless `start` is a table."""

    def __init__(self, env, action, next, start=0, validate=True):
        a, nx = _int_array(action, "action"), _int_array(next, "next")
        n_obs, n_act = int(env.observation_space.n), int(env.action_space.n)
        if a.ndim != 1 or a.shape[0] < 1:
            raise ValueError("Controller: action must have shape (K,) with K >= 1, got %s" % (a.shape,))
        K = a.shape[0]
        if nx.shape != (K, n_obs):
            raise ValueError("Controller: next must have shape (%d, %d) = (nodes, the env's observations), got %s" % (K, n_obs, nx.shape))
        if K > MAX_NODES or K * n_obs > MAX_EDGES:
            raise ValueError("Controller: %d nodes x %d observations is past the limits (%d nodes, %d successors)"
                             % (K, n_obs, MAX_NODES, MAX_EDGES))
        if validate:
            bad = _first_outside(a, n_act)
            if bad is not None:
                raise ValueError("Controller: action[%d] = %d is outside [0, %d)" % (bad[0], a[bad], n_act))
            bad = _first_outside(nx, K)
            if bad is not None:
                raise ValueError("Controller: next[%d][%d] = %d is outside [0, %d)" % (bad[0], bad[1], nx[bad], K))
        self.env = env
        self.n_nodes, self.n_obs = K, n_obs
        self.validate = bool(validate)
        self.device = env.device
        self.action = torch.as_tensor(_as_int32(a), device=self.device)
        self.next = torch.as_tensor(_as_int32(nx), device=self.device).contiguous()
        self._init_nodes(start)

    def _native_call(self):
        """(the C entry point's name, its controller argument) of env.run_controller"""
        from . import _native
        return "pomdp_controller_episodes", _native.Controller(action=self.action.data_ptr(), next=self.next.data_ptr(),
                                                               n_nodes=self.n_nodes, n_obs=self.n_obs, node=self.node.data_ptr())

    # ---- building controllers -----------------------------------------------------------------------------------------------
    @classmethod
    def concat(cls, env, parts, validate=True):
        """The disjoint union of the controllers `parts` = [(action, next), ...]: (controller, offsets) — part m's node q is
        node offsets[m] + q of the union, its successors shifted with it.  A population of M controllers is evaluated in one
        run_controller call by giving lane i the start node offsets[i % M] (plus the part's own start node)."""
        acts, nexts, offsets, K = [], [], [], 0
        for m, (action, next) in enumerate(parts):
            a, nx = _int_array(action, "action of part %d" % m), _int_array(next, "next of part %d" % m)
            if a.ndim != 1 or nx.ndim != 2 or nx.shape[0] != a.shape[0]:
                raise ValueError("Controller.concat: part %d has action %s and next %s" % (m, a.shape, nx.shape))
            if validate:
                bad = _first_outside(nx, a.shape[0])
                if bad is not None:
                    raise ValueError("Controller.concat: next[%d][%d] = %d of part %d is outside [0, %d)"
                                     % (bad[0], bad[1], nx[bad], m, a.shape[0]))
            offsets.append(K)
            acts.append(a)
            nexts.append(nx + K)
            K += a.shape[0]
        if not acts:
            raise ValueError("Controller.concat: no parts")
        return cls(env, np.concatenate(acts), np.concatenate(nexts, axis=0), validate=validate), offsets

    @classmethod
    def memoryless(cls, env, table, first_action):
        """The policy `action = table[last observation]` (table: int [n_obs]), the first step taking `first_action`: node o
        holds table[o], every node moves to the node of what it observes, and the start node (n_obs) holds first_action."""
        n_obs = int(env.observation_space.n)
        table = _int_array(table, "table")
        if table.shape != (n_obs,):
            raise ValueError("Controller.memoryless: table must have shape (%d,), got %s" % (n_obs, table.shape))
        action = np.concatenate([table, [int(first_action)]])
        return cls(env, action, np.tile(np.arange(n_obs), (len(action), 1)), start=n_obs)

    @classmethod
    def open_loop(cls, env, actions, loop=False):
        """The plan `actions` (int [K]) whatever is observed: node s holds actions[s] and moves to node s + 1; the last node
        stays on itself (its action is repeated), or with loop=True goes back to node 0 (a periodic plan)."""
        a = _int_array(actions, "actions").reshape(-1)
        succ = np.minimum(np.arange(1, len(a) + 1), len(a) - 1) if not loop else np.arange(1, len(a) + 1) % max(len(a), 1)
        return cls(env, a, np.repeat(succ[:, None], int(env.observation_space.n), axis=1))

    def __repr__(self):
        return "<Controller %s: %d nodes x %d observations, %d lanes>" % (
            getattr(self.env, "env_name", "?"), self.n_nodes, self.n_obs, self.node.shape[0])
