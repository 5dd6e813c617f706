"""ParticleBelief — a particle belief per root (lane) of a batched env, filtered on the device (include/pomdp_hip.h:
pomdp_particle_init / pomdp_particle_update), the belief a POMCP-style planner keeps per real episode.  `env.plan(belief=b)`
plans from its particles instead of from the true state."""
import numpy as np
import torch

from . import _native

# the belief's default seed: the env's seed plus this constant (mod 2^64).  A belief keyed like its env would replay the
# env's draws: particle 0 of root 0 is global lane 0 at the same call counters.
BELIEF_SEED_OFFSET = 0x9E3779B97F4A7C15


class ParticleBelief(object):
    """P particles per root of `env` (R = env.batch_size roots): `particles` is int32 [state_words, R * P], the env's state
    packing, column r * P + j = particle j of root r, global lane (env.lane_offset * P) + r * P + j.

    reset(ob, where=None): every root (or the roots with where[r] != 0) draws P fresh episodes from the env's reset() and keeps
    the ones whose reset observation equals ob[r] (ob=None: all) — the filter below.
    update(action, ob, reward=None, done=None, match_reward=False): every particle of root r is stepped under action[r]
    (pomdp_<env>_step without auto-reset); the ones that reproduce ob[r] (and done[r] when given, and reward[r] bit for bit
    with match_reward) survive, the others are redrawn uniformly from the survivors.  A root with no survivor keeps its
    proposals unfiltered ("depleted": n_match == 0); a root whose action is out of range (a plan's best == -1) is left as it
    was (n_match == -1).  Both return n_match, int32 [R] (a python int for batch_size == 1).

    The belief has its own seed (default: the env's seed + BELIEF_SEED_OFFSET mod 2^64) and its own call counter: reset() is
    call t, the first update() call t + 1, like the env's reset() and step().  Two particle buffers are used in turn, so a
    call allocates nothing on the device."""

    def __init__(self, env, n_particles=256, seed=None):
        P = int(n_particles)
        if P < 4 or P > 4096 or P % 4:
            raise ValueError("n_particles must be a multiple of 4 in [4, 4096], got %d" % P)
        R = env.batch_size
        lane0 = env.lane_offset * P
        if lane0 + R * P > 1 << 32:
            raise ValueError("the particles' global lanes (lane_offset * P + r * P + j) must lie in [0, 2^32)")
        self.env = env
        self.n_particles = P
        self.n_roots = R
        self.lane0 = lane0
        self.seed = (env._seed + BELIEF_SEED_OFFSET) & 0xFFFFFFFFFFFFFFFF if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self._t = 0
        self.device = env.device
        self._kind = _native.ENV_KIND[env.env_name]
        self._lib = _native.lib()
        self._bufs = [torch.zeros((env.state_words, R * P), dtype=torch.int32, device=self.device) for _ in range(2)]
        self._cur = 0
        self.n_match = torch.full((R,), -1, dtype=torch.int32, device=self.device)

    # ---- state -------------------------------------------------------------------------------------------------------------
    @property
    def particles(self):
        """int32 [state_words, R * P] (the live buffer: the next update() writes the other one)"""
        return self._bufs[self._cur]

    @property
    def depleted(self):
        """bool [R]: the roots whose last filter found no particle that matched"""
        return self.n_match == 0

    @property
    def call_counter(self):
        return self._t

    @call_counter.setter
    def call_counter(self, t):
        self._t = int(t)

    def set_particles(self, particles):
        """Overwrite the particles, int32 [state_words, R * P] (checked like env.set_state)."""
        self.particles.copy_(self.env._checked_state(particles, self.n_roots * self.n_particles, "set_particles", validate=True))

    def _shape_ok(self, env):
        return (env.env_name == self.env.env_name and env.batch_size == self.n_roots and env.state_words == self.env.state_words
                and bytes(env._params) == bytes(self.env._params))

    # ---- per-root arguments ------------------------------------------------------------------------------------------------
    def _col(self, x, dtype, what):
        """a per-root argument (tensor, array, list, python scalar for batch_size == 1) as a contiguous device tensor [R]:
        int32 (actions, observations: a value outside int32 becomes -1), uint8 flags (!= 0) or the env's reward dtype"""
        t = x.to(self.device) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), device=self.device)
        t = t.reshape(-1)
        if t.shape != (self.n_roots,):
            raise AssertionError("%s must have shape (%d,), got %s" % (what, self.n_roots, tuple(t.shape)))
        if dtype == torch.uint8:
            t = t != 0
        elif dtype == torch.int32 and t.dtype != torch.int32:
            if t.dtype.is_floating_point:
                raise AssertionError("%s must hold integers" % what)
            t = torch.where((t < -(1 << 31)) | (t >= 1 << 31), torch.full_like(t, -1), t)
        return t.to(dtype).contiguous()

    def _result(self):
        return int(self.n_match.item()) if self.n_roots == 1 else self.n_match

    # ---- the filter --------------------------------------------------------------------------------------------------------
    def reset(self, ob=None, where=None):
        """pomdp_particle_init: P fresh episodes per root, filtered by the reset observation ob[r] (None: no filter); with
        `where` only those roots (the others keep their particles, n_match == -1).  Returns n_match."""
        obt = None if ob is None else self._col(ob, torch.int32, "ob")
        wt = None if where is None else self._col(where, torch.uint8, "where")
        t = self._t
        self._t += 1
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_particle_init(self._kind, self.env._params_ref, self.particles.data_ptr(),
                                               None if obt is None else obt.data_ptr(), None if wt is None else wt.data_ptr(),
                                               self.n_match.data_ptr(), self.n_roots, self.n_particles, self.seed, self.lane0, t,
                                               self.env._stream())
            _native.check(rc, "pomdp_particle_init")
        return self._result()

    def update(self, action, ob, reward=None, done=None, match_reward=False):
        """pomdp_particle_update: step every particle of root r under action[r], keep those that reproduce ob[r] (and
        done[r], and reward[r] with match_reward), redraw the rest from them.  Returns n_match."""
        at = self._col(action, torch.int32, "action")
        obt = self._col(ob, torch.int32, "ob")
        dt = None if done is None else self._col(done, torch.uint8, "done")
        rt = None
        if match_reward:
            if reward is None:
                raise ValueError("update: match_reward needs the reward")
            rt = self._col(reward, torch.float32 if self.env.reward_dtype == torch.float32 else torch.int32, "reward")
        t = self._t
        self._t += 1
        src, dst = self._bufs[self._cur], self._bufs[1 - self._cur]
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_particle_update(
                self._kind, self.env._params_ref, src.data_ptr(), dst.data_ptr(), at.data_ptr(), obt.data_ptr(),
                None if rt is None else rt.data_ptr(), None if dt is None else dt.data_ptr(), self.n_match.data_ptr(),
                self.n_roots, self.n_particles, _native.PARTICLE_MATCH_REWARD if match_reward else 0, self.seed, self.lane0, t,
                self.env._stream())
            _native.check(rc, "pomdp_particle_update")
        self._cur = 1 - self._cur
        return self._result()

    def __repr__(self):
        return "<ParticleBelief %s: %d roots x %d particles>" % (self.env.env_name, self.n_roots, self.n_particles)

