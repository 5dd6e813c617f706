"""StochasticController — a stochastic finite-state controller for a batched env: node q draws its action from psi(a | q) and,
having observed ob, its successor from eta(q' | q, ob).  `env.run_controller(ctrl, steps)` plays the batch's episodes under it
inside one fused loop on the device (include/pomdp_hip.h: pomdp_stoch_controller_episodes); the draws are the lane's own Philox
words of stream CONTROLLER at (seed, lane, t), so a run reproduces under any sharding and chunking.  What bounded policy
iteration, EM, policy gradients on controllers and epsilon-soft exploration policies optimise is of this form."""
import numpy as np
import torch

from .controller import MAX_NODES, _LaneNodes, _as_int32, _first_outside, _int_array

MAX_BYTES = 36864         # include/pomdp_hip.h: POMDP_STOCH_CONTROLLER_MAX_BYTES


def footprint(K, n_obs, B, D):
    """the LDS bytes of a controller's tables: actions as bytes, successors as halfwords, thresholds as words, rounded up to 16"""
    return (K * B + 4 * K * (B - 1) + 2 * K * n_obs * D + 4 * K * n_obs * (D - 1) + 15) // 16 * 16


def quantise(p):
    """float probabilities [..., cand] -> uint32 thresholds [..., cand - 1]: thr[j] = max(0, ceil(2^32 c_j) - 1) with c_j the
    float64 cumulative sum through candidate j, clipped to 1 (the class docstring)"""
    c = np.minimum(np.cumsum(np.asarray(p, np.float64), axis=-1), 1.0)[..., :-1]
    return np.maximum(np.ceil(c * 4294967296.0) - 1.0, 0.0).astype(np.uint64).astype(np.uint32)


def _prob_array(x, what, shape):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype.kind not in "fiu" or a.shape != shape:
        raise ValueError("StochasticController: %s must hold numbers of shape %s, got dtype %s, shape %s" % (what, shape, a.dtype, a.shape))
    return a.astype(np.float64)


def _check_rows(p, what):
    """every row >= 0, sums to 1 within 1e-9, and no zero-probability candidate in front of a positive one"""
    idx = lambda t: "".join("[%d]" % v for v in t)
    bad = np.argwhere(~(p >= 0))
    if len(bad):
        raise ValueError("StochasticController: %s%s = %r is negative or NaN" % (what, idx(bad[0]), float(p[tuple(bad[0])])))
    bad = np.argwhere(~(np.abs(p.sum(axis=-1) - 1.0) <= 1e-9))
    if len(bad):
        raise ValueError("StochasticController: row %s%s sums to %r, not 1" % (what, idx(bad[0]), float(p.sum(axis=-1)[tuple(bad[0])])))
    if p.shape[-1] > 1:
        bad = np.argwhere(p[..., 0] == 0)
        if len(bad):
            raise ValueError("StochasticController: %s%s[0] = 0 stands in front of a positive candidate and would be drawn with "
                             "probability 2^-32 — put padding last" % (what, idx(bad[0])))


def _thr_array(x, what, shape):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.size == 0:
        a = np.zeros(shape, np.uint32)
    if a.dtype.kind not in "iu" or a.shape != shape or (a.astype(np.int64) < 0).any() or (a.astype(np.uint64) >> 32).any():
        raise ValueError("StochasticController: %s must hold uint32 values of shape %s" % (what, shape))
    return a.astype(np.uint32)


class StochasticController(_LaneNodes):
    """StochasticController(env, action, action_p, next, next_p, start=0, validate=True)

    Candidate form: K nodes; action int [K, B] — the B candidate actions of node q — with action_p float [K, B], their
    probabilities psi; next int [K, n_obs, D] — the D candidate successors of node q on observation o — with next_p float
    [K, n_obs, D], their probabilities eta.  Every probability row is >= 0 and sums to 1 within 1e-9.  B = D = 1 is the
    deterministic Controller.  1 <= K <= 4096, and the tables' LDS footprint K*B + 4*K*(B-1) + 2*K*n_obs*D + 4*K*n_obs*(D-1)
    (rounded up to 16) is at most 36864 bytes.

    Quantisation: the kernel picks in integers.  With c_j the float64 cumulative sum of a row through candidate j, clipped to
    1, thr[j] = max(0, ceil(2^32 c_j) - 1) for j < candidates - 1, and the candidate drawn by a 32-bit word u is the number of
    j with u > thr[j].  So candidate 0 is drawn with probability ceil(2^32 c_0) / 2^32, every probability is within 2^-32 of
    the stated one, and a probability of exactly 1 is exact.  A zero-probability candidate IN FRONT of a positive one would be
    drawn with probability 2^-32 instead of 0; validate=True refuses it — put padding last (from_dense sorts it there).

    validate=True also checks every candidate action in [0, n_actions) and every candidate successor in [0, K), as Controller
    does.  validate=False skips the checks and takes the raw thresholds — action_thr= uint32 [K, B - 1] and next_thr= uint32
    [K, n_obs, D - 1] — in place of probabilities (action_p / next_p may then be None); the kernel treats a refused entry
    as the header says, counted in env.invalid_action_count().

    start, reset_nodes(ob=, where=) and node: exactly as on Controller.  `action`, `next` (int32), `action_thr`, `next_thr`
    (uint32 values in int32 tensors' bits) and `node` are the tensors the kernel reads."""

    def __init__(self, env, action, action_p, next, next_p, start=0, validate=True, action_thr=None, next_thr=None):
        a, nx = _int_array(action, "action"), _int_array(next, "next")
        n_obs, n_act = int(env.observation_space.n), int(env.action_space.n)
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("StochasticController: action must have shape (K, B) with K, B >= 1, got %s" % (a.shape,))
        K, B = a.shape
        if nx.ndim != 3 or nx.shape[:2] != (K, n_obs) or nx.shape[2] < 1:
            raise ValueError("StochasticController: next must have shape (%d, %d, D) = (nodes, the env's observations, candidates), "
                             "got %s" % (K, n_obs, nx.shape))
        D = nx.shape[2]
        if K > MAX_NODES or footprint(K, n_obs, B, D) > MAX_BYTES:
            raise ValueError("StochasticController: %d nodes x %d observations with %d action and %d successor candidates is past "
                             "the limits (%d nodes, %d bytes of tables; these need %d)"
                             % (K, n_obs, B, D, MAX_NODES, MAX_BYTES, footprint(K, n_obs, B, D)))
        if (action_thr is not None or next_thr is not None) and validate:
            raise ValueError("StochasticController: raw thresholds are taken with validate=False only")
        thr = []
        for raw, p, what, shape in ((action_thr, action_p, "action", (K, B)), (next_thr, next_p, "next", (K, n_obs, D))):
            if raw is not None:
                thr.append(_thr_array(raw, what + "_thr", shape[:-1] + (shape[-1] - 1,)))
                continue
            if p is None:
                raise ValueError("StochasticController: %s_p is missing" % what)
            p = _prob_array(p, what + "_p", shape)
            if validate:
                _check_rows(p, what + "_p")
            thr.append(quantise(p))
        if validate:
            bad = _first_outside(a, n_act)
            if bad is not None:
                raise ValueError("StochasticController: action[%d][%d] = %d is outside [0, %d)" % (bad + (a[bad], n_act)))
            bad = _first_outside(nx, K)
            if bad is not None:
                raise ValueError("StochasticController: next[%d][%d][%d] = %d is outside [0, %d)" % (bad + (nx[bad], K)))
        self.env = env
        self.n_nodes, self.n_obs, self.n_act_cand, self.n_next_cand = K, n_obs, B, D
        self.validate = bool(validate)
        self.device = env.device
        self.action = torch.as_tensor(_as_int32(a), device=self.device).contiguous()
        self.next = torch.as_tensor(_as_int32(nx), device=self.device).contiguous()
        self.action_thr = torch.as_tensor(thr[0].view(np.int32), device=self.device).contiguous()
        self.next_thr = torch.as_tensor(thr[1].view(np.int32), device=self.device).contiguous()
        self._init_nodes(start)

    def _native_call(self):
        """(the C entry point's name, its controller argument) of env.run_controller"""
        from . import _native
        return "pomdp_stoch_controller_episodes", _native.StochController(
            action=self.action.data_ptr(), action_thr=self.action_thr.data_ptr() if self.n_act_cand > 1 else None,
            next=self.next.data_ptr(), next_thr=self.next_thr.data_ptr() if self.n_next_cand > 1 else None,
            n_nodes=self.n_nodes, n_obs=self.n_obs, n_act_cand=self.n_act_cand, n_next_cand=self.n_next_cand, node=self.node.data_ptr())

    # ---- building controllers -----------------------------------------------------------------------------------------------
    @classmethod
    def from_dense(cls, env, psi, eta, start=0):
        """psi float [K, n_actions], eta float [K, n_obs, K] -> B = n_actions, D = K: every action and every node a candidate,
        each row's candidates in order of falling probability (ties by index), so that zero-probability entries come last"""
        n_act, n_obs = int(env.action_space.n), int(env.observation_space.n)
        psi = np.asarray(psi.detach().cpu().numpy() if isinstance(psi, torch.Tensor) else psi, np.float64)
        eta = np.asarray(eta.detach().cpu().numpy() if isinstance(eta, torch.Tensor) else eta, np.float64)
        if psi.ndim != 2 or psi.shape[1] != n_act or eta.shape != (psi.shape[0], n_obs, psi.shape[0]):
            raise ValueError("StochasticController.from_dense: psi must have shape (K, %d) and eta (K, %d, K), got %s and %s"
                             % (n_act, n_obs, psi.shape, eta.shape))
        ia, inx = np.argsort(-psi, axis=-1, kind="stable"), np.argsort(-eta, axis=-1, kind="stable")
        return cls(env, ia, np.take_along_axis(psi, ia, -1), inx, np.take_along_axis(eta, inx, -1), start=start)

    @classmethod
    def from_controller(cls, ctrl):
        """the deterministic Controller `ctrl` as a stochastic one (B = D = 1), on the same start nodes"""
        K, n_obs = ctrl.n_nodes, ctrl.n_obs
        start = ctrl.start if isinstance(ctrl.start, int) else ctrl.start.cpu().numpy()
        return cls(ctrl.env, ctrl.action.cpu().numpy()[:, None], np.ones((K, 1)), ctrl.next.cpu().numpy()[:, :, None],
                   np.ones((K, n_obs, 1)), start=start, validate=ctrl.validate)

    @classmethod
    def epsilon_soft(cls, ctrl, eps):
        """psi = (1 - eps) * delta(ctrl's action) + eps * uniform over the env's actions, ctrl's successors kept (D = 1).  Node q's
        candidates are its own action first, then the others in rising order (so eps = 0 puts the zeros last)."""
        eps = float(eps)
        if not 0.0 <= eps <= 1.0:
            raise ValueError("StochasticController.epsilon_soft: eps must lie in [0, 1], got %r" % eps)
        K, n_obs, n_act = ctrl.n_nodes, ctrl.n_obs, int(ctrl.env.action_space.n)
        own = ctrl.action.cpu().numpy().astype(np.int64)
        bad = _first_outside(own, n_act)
        if bad is not None:
            raise ValueError("StochasticController.epsilon_soft: action[%d] = %d is outside [0, %d)" % (bad[0], own[bad], n_act))
        others = np.arange(n_act)[None, :].repeat(K, 0)
        others = others[others != own[:, None]].reshape(K, n_act - 1)
        p = np.full((K, n_act), eps / n_act)
        p[:, 0] += 1.0 - eps
        start = ctrl.start if isinstance(ctrl.start, int) else ctrl.start.cpu().numpy()
        return cls(ctrl.env, np.concatenate([own[:, None], others], axis=1), p, ctrl.next.cpu().numpy()[:, :, None],
                   np.ones((K, n_obs, 1)), start=start, validate=ctrl.validate)

    @classmethod
    def concat(cls, env, parts, validate=True):
        """The disjoint union of the controllers `parts` = [(action, action_p, next, next_p), ...]: (controller, offsets), as
        Controller.concat.  Parts are padded to a common B and D with zero-probability candidates LAST (copies of the row's
        candidate 0, never drawn)."""
        if not parts:
            raise ValueError("StochasticController.concat: no parts")
        n_obs = int(env.observation_space.n)
        got = []
        for m, (action, action_p, next, next_p) in enumerate(parts):
            a, nx = _int_array(action, "action of part %d" % m), _int_array(next, "next of part %d" % m)
            if a.ndim != 2 or nx.ndim != 3 or nx.shape[:2] != (a.shape[0], n_obs):
                raise ValueError("StochasticController.concat: part %d has action %s and next %s" % (m, a.shape, nx.shape))
            if validate:
                bad = _first_outside(nx, a.shape[0])
                if bad is not None:
                    raise ValueError("StochasticController.concat: next[%d][%d][%d] = %d of part %d is outside [0, %d)"
                                     % (bad + (nx[bad], m, a.shape[0])))
            got.append((a, _prob_array(action_p, "action_p of part %d" % m, a.shape), nx,
                        _prob_array(next_p, "next_p of part %d" % m, nx.shape)))
        B, D = max(g[0].shape[1] for g in got), max(g[2].shape[2] for g in got)

        def pad(v, p, width):
            extra = width - v.shape[-1]
            return (np.concatenate([v, np.repeat(v[..., :1], extra, axis=-1)], axis=-1),
                    np.concatenate([p, np.zeros(p.shape[:-1] + (extra,))], axis=-1))
        acts, aps, nexts, nps, offsets, K = [], [], [], [], [], 0
        for a, ap, nx, nxp in got:
            a, ap = pad(a, ap, B)
            nx, nxp = pad(nx + K, nxp, D)
            offsets.append(K)
            acts.append(a), aps.append(ap), nexts.append(nx), nps.append(nxp)
            K += a.shape[0]
        return cls(env, np.concatenate(acts), np.concatenate(aps), np.concatenate(nexts), np.concatenate(nps), validate=validate), offsets

    def __repr__(self):
        return "<StochasticController %s: %d nodes x %d observations, %d action / %d successor candidates, %d lanes>" % (
            getattr(self.env, "env_name", "?"), self.n_nodes, self.n_obs, self.n_act_cand, self.n_next_cand, self.node.shape[0])

