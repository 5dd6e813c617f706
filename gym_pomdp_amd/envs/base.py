"""BatchedEnv — host-side mirror of the reference's gym.Env duck type
(`reset() -> ob`, `step(a) -> (ob, reward, done, info)`, `seed`, `action_space`,
`observation_space`; gym_pomdp/envs/rock.py:96-271 and siblings) for a batch of
independent env instances ("lanes") whose state lives in HBM as packed int32
columns and is advanced by the HIP kernels behind include/pomdp_hip.h.

Semantics added by batching:
  * lanes are globally numbered `lane_offset + i`; every random draw depends only on
    (seed, global lane, call counter t, stream id), so sharding a batch over GPUs or
    changing the launch geometry never changes a result;
  * the call counter t advances by one on every reset()/step() call;
  * `auto_reset=True` (default for batch_size > 1): a lane that reports done gets a
    fresh episode inside the same step() call — the terminal (ob, reward, done=1) is
    returned, the stored state is the new episode's;
  * `auto_reset=False` (default for batch_size == 1, the reference's behaviour): done
    lanes freeze; with batch_size == 1 stepping a done env raises AssertionError
    exactly like the reference (rock.py:126).
"""
import ctypes as C
import os

import numpy as np
import torch

from .. import _native, compat
from ..spaces import Discrete


def _random_seed():
    return int.from_bytes(os.urandom(8), "little")


def _public_raw_stream(dev_index):
    return torch.cuda.current_stream(dev_index).cuda_stream


def _resolve_fast_handles(c_module=None):
    """(raw hipStream_t of torch's current stream on a device, current device index) as plain callables.  torch keeps
    both as private C functions (no Stream object built, no device query through python); they are not a stable API, so
    they are looked up ONCE here and anything missing falls back to the public calls (tests/test_host_logic.py)."""
    c_module = torch._C if c_module is None else c_module
    raw = getattr(c_module, "_cuda_getCurrentRawStream", None)
    cur = getattr(c_module, "_cuda_getDevice", None)
    return (raw if callable(raw) else _public_raw_stream), (cur if callable(cur) else torch.cuda.current_device)


_raw_stream, _current_device = _resolve_fast_handles()


STAGGER_BYTES = 4096


def staggered(specs, device):
    """One allocation carved into the given columns — [(shape, dtype), ...] -> [tensor, ...], zero-filled — with the k-th
    column starting k * 4 KB past a 4 KB boundary of its own.  Why: separate allocations of this size all start on the same
    2 MB boundary, a kernel that touches element i of every column at the same time (every step kernel does) then keeps
    hitting the same HBM channel, and the store stream of a fused launch runs 6 % (RockSample) to 14 % (Tiger) slower than
    with the columns spread (profiles/r02d_store_layout.txt)."""
    offs, total = [], 0
    for k, (shape, dtype) in enumerate(specs):
        nbytes = int(torch.Size(shape).numel()) * torch.empty((), dtype=dtype).element_size()
        total = -(-total // STAGGER_BYTES) * STAGGER_BYTES + (k % 16) * STAGGER_BYTES
        offs.append((total, nbytes))
        total += nbytes
    pool = torch.zeros(total + STAGGER_BYTES, dtype=torch.uint8, device=device)
    return [pool[o:o + nb].view(dtype).view(shape) for (o, nb), (shape, dtype) in zip(offs, specs)]


class BatchedEnv(compat.EnvBase):
    """A `gym.Env` when an old-API gym is importable (compat.EnvBase), so that `gym.make()`'s wrappers and type checks
    accept it; either way it carries what `gym.make` touches: `unwrapped`, `spec`, `np_random`, `render_mode`, `metadata`."""
    metadata = {"render.modes": ["ansi"], "render_modes": ["ansi"]}      # gym <= 0.21 / gym >= 0.22 spelling
    reward_range = (-float("inf"), float("inf"))
    spec = None               # gym.make: `env.unwrapped.spec = spec` (gym/envs/registration.py, EnvSpec.make)
    render_mode = None
    env_name = None           # "rock", "tag", ... (C-ABI entry-point infix)
    reward_dtype = torch.int32

    # ---- subclasses provide -------------------------------------------------
    def _build_params(self):  # -> (ctypes Structure, words per lane, n_actions, n_obs)
        raise NotImplementedError

    # ---- construction ---------------------------------------------------------
    def _setup(self, batch_size=1, device=None, seed=None, auto_reset=None, lane_offset=0, reuse_buffers=False):
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if lane_offset < 0 or lane_offset + batch_size > 1 << 32:
            raise ValueError("lane range must lie in [0, 2^32)")
        self.batch_size = batch_size
        self.num_envs = batch_size
        self.lane_offset = int(lane_offset)
        self._auto_reset = (batch_size > 1) if auto_reset is None else bool(auto_reset)
        self.reuse_buffers = bool(reuse_buffers)
        self._params, self.state_words, n_actions, n_obs = self._build_params()
        self._params_ref = C.byref(self._params)
        self.action_space = Discrete(n_actions)
        self.observation_space = Discrete(n_obs)
        self._seed = _random_seed() if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self._t = 0
        self._lib = _native.lib()                       # raises if the HIP library is missing
        self._reset_fn = getattr(self._lib, "pomdp_%s_reset" % self.env_name)
        self._step_fn = getattr(self._lib, "pomdp_%s_step" % self.env_name)
        if not torch.cuda.is_available():
            raise RuntimeError("gym_pomdp_amd: no GPU visible — the batched envs run on MI355X only "
                               "(there is no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("device must be a cuda (ROCm) device, got %s" % self.device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        n = batch_size
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._state, self._ob, self._reward, self._done = staggered(
            [((self.state_words, n), torch.int32), ((n,), torch.int32), ((n,), self.reward_dtype), ((n,), torch.uint8)], self.device)
        if n == 1:
            # scalar mode (the reference's usage): the step kernel writes ob / reward / done straight into 16 bytes of
            # pinned host memory (device-visible under unified addressing), so a step is one launch + one stream
            # synchronisation, no copy; the action is passed as a pointer into a device-resident table of all action
            # values, so there is no per-step H2D copy either
            self._scalar_buf = torch.zeros(4, dtype=torch.int32, device=self.device)
            self._ob = self._scalar_buf[0:1]
            self._reward = self._scalar_buf[1:2].view(self.reward_dtype)
            self._done = self._scalar_buf[2:3].view(torch.uint8)[0:1]
            self._action_table = torch.arange(n_actions, dtype=torch.int32, device=self.device)
            self._host_out = torch.zeros(4, dtype=torch.int32).pin_memory()
            self._host_reward = self._host_out[1:2].view(self.reward_dtype)
            self._host_ob_t = self._host_out[0:1]
            self._host_done_t = self._host_out[2:3].view(torch.uint8)[0:1]
            hp = self._host_out.data_ptr()
            self._host_ptrs = (hp, hp + 4, hp + 8)
            self._host_np = self._host_out.numpy()                       # same memory, cheap scalar reads
            self._host_reward_np = self._host_reward.numpy()
            self._action_base = self._action_table.data_ptr()
        self._has_reset = False
        self._last_reset = None
        self._scalar_done = False
        self._dev_flags_used = False    # a C-side driver wrote the device-side ob / done of a scalar env (see reset())
        self._collect_cache = {}        # collect_synthetic: bound argument structs by (buffer pointers, steps)
        self._tracker = None          # per-step side effects beyond (state, ob, reward, done): RockSample's side statistics
        self._done_bool = self._done.view(torch.bool)
        self._ptrs = (self._state.data_ptr(), self._ob.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(),
                      self._err.data_ptr())
        # everything of a step() call that does not change between calls, bound once (include/pomdp_hip.h: pomdp_step_args)
        self._step_args = _native.StepArgs(
            env=_native.ENV_KIND[self.env_name], flags=_native.POMDP_AUTO_RESET if self._auto_reset else 0,
            params=C.addressof(self._params), state=self._ptrs[0], ob=self._ptrs[1], reward=self._ptrs[2],
            done=self._ptrs[3], err=self._ptrs[4], n=n, seed=self._seed, lane0=self.lane_offset, reserved=0)
        self._step_args_ref = C.byref(self._step_args)
        self._bound_step = self._lib.pomdp_step
        if n == 1:                       # scalar mode: the same call with ob / reward / done in pinned host memory
            self._scalar_args = _native.StepArgs(
                env=self._step_args.env, flags=self._step_args.flags, params=C.addressof(self._params), state=self._ptrs[0],
                ob=self._host_ptrs[0], reward=self._host_ptrs[1], done=self._host_ptrs[2], err=self._ptrs[4], n=1,
                seed=self._seed, lane0=self.lane_offset, reserved=0)
            self._scalar_args_ref = C.byref(self._scalar_args)
            self._bound_step_sync = self._lib.pomdp_step_sync
        self._action_shape = torch.Size((n,))
        self._dev_index = self.device.index
        self._info = {"state": self._state}

    @property
    def unwrapped(self):
        """gym.Env.unwrapped: the env under every wrapper — this object."""
        return self

    @property
    def np_random(self):
        """gym.Env.np_random (gym >= 0.22 keeps one per env).  The kernels never draw from it — their words are Philox
        streams of (seed, lane, t) — it exists for callers and wrappers that expect the attribute."""
        rng = self.__dict__.get("_np_random")
        if rng is None:
            rng = self.__dict__["_np_random"] = np.random.RandomState(getattr(self, "_seed", 0) & 0xFFFFFFFF)
        return rng

    @np_random.setter
    def np_random(self, value):
        self.__dict__["_np_random"] = value

    @property
    def auto_reset(self):
        return self._auto_reset

    @auto_reset.setter
    def auto_reset(self, value):
        if self._auto_reset and not value and self.batch_size > 1:
            # without auto-reset `done` is in/out (a set flag freezes the lane); what the buffer holds now are the flags the
            # last auto-resetting step RETURNED, and those lanes have fresh episodes
            self._done.zero_()
        self._auto_reset = bool(value)
        self._step_args.flags = _native.POMDP_AUTO_RESET if self._auto_reset else 0
        if self.batch_size == 1:
            self._scalar_args.flags = self._step_args.flags

    # ---- gym.Env surface --------------------------------------------------------
    def seed(self, seed=None):
        """Reference: np.random.seed(seed) on the global stream (rock.py:120-121).  Here: the
        Philox key of this env's lanes; the call counter restarts."""
        self._seed = _random_seed() if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self._step_args.seed = self._seed
        if self.batch_size == 1:
            self._scalar_args.seed = self._seed
        self._t = 0
        self.__dict__.pop("_np_random", None)
        return [self._seed]

    @property
    def call_counter(self):
        """t of the next reset()/step() call (the Philox counter word pair)."""
        return self._t

    @call_counter.setter
    def call_counter(self, t):
        self._t = int(t)

    def _stream(self):
        """hipStream_t of torch's current stream on this env's device (the raw handle: no Stream object is built)."""
        return _raw_stream(self._dev_index)

    def reset(self, *, seed=None, options=None, return_info=False, where=None):
        """All lanes start a new episode.  Returns ob: int32[N] tensor (python int if batch_size == 1).
        The reference's reset() takes no arguments; the keywords are what gym 0.22-0.25's `gym.make` wrappers pass through
        (`seed`: seed(seed) first; `return_info`: (ob, info) instead of ob; `options` is accepted and ignored).
        `where` (bool / uint8 [N], e.g. env.done): only those lanes start a new episode — the one reset() at this call counter
        would give them — and have their done flag cleared; every other lane keeps its state and done flag and reports
        ob = -1 (pomdp_reset_where).  The call counter advances by one either way."""
        if seed is not None:
            self.seed(seed)
        if return_info:
            return self.reset(where=where), self._info
        if where is not None:
            return self._reset_where(where)
        t = self._t
        self._t += 1
        if self.batch_size == 1 and not self._dev_flags_used and _current_device() == self._dev_index:
            # scalar mode: the observation goes straight to pinned host memory; launch and wait in one FFI call, read.
            # Only while nothing has written the DEVICE-side ob / done of this env: heuristic_steps() and
            # rollout_synthetic() take the device done flag as an in/out freeze flag, so after them the general path
            # below runs once (it clears that flag and refreshes the device-side observation)
            rc = self._lib.pomdp_reset_sync(self._step_args.env, self._params_ref, self._ptrs[0], self._host_ptrs[0], 1, self._seed,
                                            self.lane_offset, t, _raw_stream(self._dev_index))
            _native.check(rc, "pomdp_%s_reset" % self.env_name)
            self._host_out[2] = 0
            if self._tracker is not None:
                self._tracker.on_reset()
            ob = int(self._host_np[0])
            self._has_reset, self._scalar_done, self.done = True, False, False
            self._last_reset = (ob, t)
            return ob
        with torch.cuda.device(self.device):
            ob = self._ob if self.reuse_buffers else torch.empty_like(self._ob)
            rc = self._reset_fn(self._params_ref, self._state.data_ptr(), ob.data_ptr(), self.batch_size,
                                self._seed, self.lane_offset, t, self._stream())
            _native.check(rc, "pomdp_%s_reset" % self.env_name)
            self._done.zero_()
            if self.batch_size == 1:
                self._host_out[2] = 0            # the done flag the scalar step keeps in pinned host memory
            if self._tracker is not None:
                self._tracker.on_reset()
        self._has_reset = True
        self._scalar_done = False
        self._dev_flags_used = False
        self._last_reset = (ob, t)      # History() picks the current observation up from here
        self.done = False if self.batch_size == 1 else self._done.view(torch.bool)
        if self.batch_size == 1:
            return int(ob.item())
        return ob

    def _reset_where(self, where):
        """reset(where=...): the masked reset of the lanes with where[i] != 0."""
        if not self._has_reset:
            raise AttributeError("%s: reset(where=...) before reset()" % type(self).__name__)
        n = self.batch_size
        if n == 1:
            w = where.item() if isinstance(where, torch.Tensor) else np.asarray(where).reshape(-1)[0]
            if bool(w):
                return self.reset()
            self._t += 1
            return -1
        mask = self._as_lane_mask(where)
        t = self._t
        self._t += 1
        with torch.cuda.device(self.device):
            ob = self._ob if self.reuse_buffers else torch.empty_like(self._ob)
            rc = self._lib.pomdp_reset_where(self._step_args.env, self._params_ref, self._ptrs[0], ob.data_ptr(), self._ptrs[3],
                                             mask.data_ptr(), n, self._seed, self.lane_offset, t, self._stream())
            _native.check(rc, "pomdp_reset_where")
            if self._tracker is not None:
                self._tracker.on_reset(mask)
        self._last_reset = None         # not every lane's observation is a fresh episode's
        self.done = self._done.view(torch.bool)
        return ob

    def _as_lane_mask(self, where):
        """a per-lane mask (bool / integer [N], any device) as the uint8 tensor on this env's device the kernels read"""
        if isinstance(where, torch.Tensor):
            if where.dtype.is_floating_point:
                raise AssertionError("a lane mask must be bool or integer")
            m = where.to(self.device)
        else:
            arr = np.asarray(where)
            if arr.dtype.kind not in "biu":
                raise AssertionError("a lane mask must be bool or integer")
            m = torch.as_tensor(arr, device=self.device)
        if m.shape != (self.batch_size,):
            raise AssertionError("a lane mask must have shape (%d,), got %s" % (self.batch_size, tuple(m.shape)))
        if m.dtype != torch.uint8:
            m = (m != 0).to(torch.uint8)
        return m.contiguous()

    def step(self, action):
        """action: int32[N] tensor on this env's device (other integer tensors / arrays / lists are
        converted); python int when batch_size == 1.  Returns (ob, reward, done, info) like the
        reference, as tensors (python scalars when batch_size == 1); info["state"] aliases the live
        packed state, as the reference's info["state"] aliases live internals."""
        if not self._has_reset:
            # the reference raises AttributeError here: `self.done` does not exist before reset()
            raise AttributeError("%s: step() called before reset()" % type(self).__name__)
        if self.batch_size == 1:
            assert self.action_space.contains(action), "invalid action %r" % (action,)
            assert self._scalar_done is False or self._auto_reset, "step() on a done env (call reset())"
            return self._scalar_step(int(action))
        if not (type(action) is torch.Tensor and action.dtype is torch.int32 and action.shape == self._action_shape
                and action.device == self.device and action.is_contiguous()):
            action = self._as_action_tensor(action)           # slow path: convert / validate
        t = self._t
        self._t = t + 1
        if self.reuse_buffers and _current_device() == self._dev_index:
            # hot path: one FFI call with four arguments (the rest is bound in self._step_args), no allocation, no
            # device-context switch, the raw stream handle
            rc = self._bound_step(self._step_args_ref, action.data_ptr(), t, _raw_stream(self._dev_index))
            if rc:
                _native.check(rc, "pomdp_%s_step" % self.env_name)
            if self._tracker is not None:
                self._tracker.on_step(action, self._ob, self._done, self._step_args.flags)
            self.done = self._done_bool
            return self._ob, self._reward, self._done_bool, self._info
        flags = _native.POMDP_AUTO_RESET if self._auto_reset else 0
        with torch.cuda.device(self.device):
            if self.reuse_buffers:
                ob, reward = self._ob, self._reward
            else:
                ob, reward = torch.empty_like(self._ob), torch.empty_like(self._reward)
            done = self._done if (self.reuse_buffers or not self._auto_reset) else torch.empty_like(self._done)
            rc = self._step_fn(self._params_ref, self._state.data_ptr(), action.data_ptr(), ob.data_ptr(),
                               reward.data_ptr(), done.data_ptr(), self._err.data_ptr(), self.batch_size,
                               self._seed, self.lane_offset, t, flags, self._stream())
            _native.check(rc, "pomdp_%s_step" % self.env_name)
        if not self._auto_reset and not self.reuse_buffers:
            done = done.clone()
        if self._tracker is not None:
            self._tracker.on_step(action, ob, done, flags)
        self.done = self._done_bool if done is self._done else done.view(torch.bool)
        return ob, reward, self.done, self._info

    def _scalar_step(self, action):
        """batch_size == 1: one launch writing into pinned host memory and one stream synchronisation — both inside ONE
        FFI call (pomdp_step_sync) — python scalars out."""
        t = self._t
        self._t = t + 1
        if self._tracker is None and _current_device() == self._dev_index:
            rc = self._bound_step_sync(self._scalar_args_ref, self._action_base + 4 * action, t,
                                       _raw_stream(self._dev_index))
            if rc:
                _native.check(rc, "pomdp_%s_step" % self.env_name)
        else:
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream(self.device)
                rc = self._bound_step(self._scalar_args_ref, self._action_base + 4 * action, t, stream.cuda_stream)
                if rc:
                    _native.check(rc, "pomdp_%s_step" % self.env_name)
                if self._tracker is not None:
                    self._tracker.on_step(self._action_table[action:action + 1], self._host_ob_t, self._host_done_t,
                                          self._scalar_args.flags)
                stream.synchronize()
        h = self._host_np
        d = bool(h[2] & 0xFF)
        self._scalar_done = d
        self.done = d
        r = self._host_reward_np[0]
        return int(h[0]), (int(r) if self.reward_dtype == torch.int32 else float(r)), d, self._info

    def _as_action_tensor(self, action):
        if isinstance(action, torch.Tensor):
            if action.dtype.is_floating_point or action.dtype == torch.bool:
                raise AssertionError("actions must be integers")
            if action.dtype != torch.int32:
                # a wider value must not wrap into a valid action (2^32 + 1 -> 1): anything outside the action space
                # becomes -1, which the kernels count as invalid and ignore (the reference asserts, rock.py:125)
                action = torch.where((action < 0) | (action >= self.action_space.n), torch.full_like(action, -1), action)
            a = action.to(device=self.device, dtype=torch.int32)
        else:
            arr = np.asarray(action)
            if arr.dtype.kind not in "iu":
                raise AssertionError("actions must be integers")
            if arr.dtype != np.int32:
                arr = np.where((arr < 0) | (arr >= self.action_space.n), -1, arr)
            a = torch.as_tensor(arr.astype(np.int32), device=self.device)
        if a.shape != (self.batch_size,):
            raise AssertionError("actions must have shape (%d,), got %s" % (self.batch_size, tuple(a.shape)))
        return a.contiguous()

    def render(self, mode="ansi", close=False):
        if close:
            return
        raise NotImplementedError("rendering is out of scope for the batched envs (SURVEY.md §2: GUI)")

    def close(self):
        return

    # ---- batch-side extras --------------------------------------------------------
    @property
    def state(self):
        """Packed lane state, int32 [state_words, N] (layout: include/pomdp_hip.h)."""
        return self._state

    def set_state(self, state):
        """Overwrite the packed lane state (planner hook `_set_state`; tensor copy).  `state` is int32
        [state_words, N] (or [N] / a scalar-mode [state_words] for one-word layouts): anything else is rejected, so a
        state saved under another layout (BattleShip had 2 * MW words before ABI 10) cannot be misread."""
        self._state.copy_(self._checked_state(state, self.batch_size, "set_state", validate=True))
        self._done.zero_()
        if self.batch_size == 1:
            self._host_out[2] = 0
        self._scalar_done = False
        self._has_reset = True
        self.done = False if self.batch_size == 1 else self._done.view(torch.bool)
        if self._tracker is not None:
            self._tracker.on_reset()

    _set_state = set_state

    def _checked_state(self, state, lanes, what, validate=False):
        """`state` as an int32 [state_words, lanes or -1] device tensor, shape-checked (lanes=None: any lane count);
        validate: also the env's own sanity check of a state that is going to be stepped."""
        st = torch.as_tensor(state, dtype=torch.int32, device=self.device)
        if st.dim() == 1 and (self.state_words == 1 or (lanes == 1 and st.numel() == self.state_words)):
            st = st.reshape(self.state_words, -1)
        if st.dim() != 2 or st.shape[0] != self.state_words or (lanes is not None and st.shape[1] != lanes):
            raise ValueError("%s: expected a packed state of shape (%d, %s), got %s" % (
                what, self.state_words, "N" if lanes is None else lanes, tuple(st.shape)))
        if validate:
            self._validate_state(st, what)
        return st.contiguous()

    def _validate_state(self, st, what):
        """env-specific sanity of a caller-supplied packed state (BattleShip: the cached next board)"""
        return

    def invalid_action_count(self):
        """Lanes that were handed an out-of-range action since construction (they were left
        untouched; the reference would have raised AssertionError).  Synchronises."""
        return int(self._err.item())

    def synthetic_actions(self, out=None, seed=None):
        """Uniform random actions from the bench's synthetic policy (stream ACTION of the *current* call
        counter); int32[N] on device.  lane_offset must be a multiple of 4."""
        if self.lane_offset % 4:
            raise ValueError("synthetic_actions: lane_offset must be a multiple of 4 (got %d)" % self.lane_offset)
        if out is None:
            out = torch.empty(self.batch_size, dtype=torch.int32, device=self.device)
        if torch.cuda.current_device() == self.device.index:
            rc = self._lib.pomdp_synthetic_actions(out.data_ptr(), self.batch_size,
                                                   self._seed if seed is None else seed, self.lane_offset,
                                                   self._t, self.action_space.n, self._stream())
            if rc:
                _native.check(rc, "pomdp_synthetic_actions")
            return out
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_synthetic_actions(out.data_ptr(), self.batch_size,
                                                   self._seed if seed is None else seed, self.lane_offset,
                                                   self._t, self.action_space.n, self._stream())
            _native.check(rc, "pomdp_synthetic_actions")
        return out

    # ---- planner hooks (reference: _get_init_state / _set_state / _generate_legal / _discount) --------
    def _get_init_state(self):
        """A fresh batch of initial states (packed int32 [state_words, N]) without touching the live
        state — the reference's `_get_init_state()` (rock.py:266-271 etc.).  Advances the call counter."""
        t = self._t
        self._t += 1
        out = torch.empty_like(self._state)
        with torch.cuda.device(self.device):
            rc = self._reset_fn(self._params_ref, out.data_ptr(), None, self.batch_size, self._seed,
                                self.lane_offset, t, self._stream())
            _native.check(rc, "pomdp_%s_reset" % self.env_name)
        return out

    def legal_actions(self, state=None):
        """`_generate_legal()` of every lane: (list int32 [N, n_actions] in the reference's order, padded
        with -1; length int32 [N]).  `state` defaults to the live state."""
        st = self._state if state is None else self._checked_state(state, None, "legal_actions")
        n = st.shape[1]
        stride = self.action_space.n
        lst = torch.empty((n, stride), dtype=torch.int32, device=self.device)
        ln = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_legal_actions(_native.ENV_KIND[self.env_name], self._params_ref, st.data_ptr(),
                                               lst.data_ptr(), ln.data_ptr(), n, stride, self._stream())
            _native.check(rc, "pomdp_legal_actions")
        return lst, ln

    def _generate_legal(self):
        """batch_size == 1: the reference's python list; otherwise the (list, length) tensors."""
        lst, ln = self.legal_actions()
        if self.batch_size == 1:
            return lst[0, : int(ln.item())].tolist()
        return lst, ln

    def preferred_actions(self, history, state=None):
        """`_generate_preferred(history)` of every lane, in the shape of legal_actions(): (list int32 [N, n_actions]
        padded with -1, length int32 [N]).  `history` is a gym_pomdp_amd.history.History of this env."""
        st = self._state if state is None else self._checked_state(state, None, "preferred_actions")
        n = st.shape[1]
        if n != self.batch_size:
            raise ValueError("preferred_actions: the history and side statistics cover exactly batch_size lanes")
        stride = self.action_space.n
        lst = torch.empty((n, stride), dtype=torch.int32, device=self.device)
        ln = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_preferred_actions(_native.ENV_KIND[self.env_name], self._params_ref, st.data_ptr(),
                                                   self._belief_ref(), history._ref, lst.data_ptr(), ln.data_ptr(), n,
                                                   stride, self._stream())
            _native.check(rc, "pomdp_preferred_actions")
        return lst, ln

    def _belief_ref(self):
        return None

    def _generate_preferred(self, history):
        """Reference signature (tag.py:231-243; tiger.py:114-115, network.py:138-139: the legal list).
        batch_size == 1: a python list; otherwise the (list, length) tensors."""
        lst, ln = self.preferred_actions(history)
        if self.batch_size == 1:
            return lst[0, : int(ln.item())].tolist()
        return lst, ln

    def pick_actions(self, lists, lengths, seed=None, out=None):
        """The caller's `np.random.choice(list)` for every lane (rock.py:564): element (w * length) >> 32 of each
        lane's list, w being the synthetic policy's word at the *current* call counter.  -> int32[N]."""
        if out is None:
            out = torch.empty(self.batch_size, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_pick_actions(lists.data_ptr(), lengths.data_ptr(), lists.shape[1], out.data_ptr(),
                                              self.batch_size, self._seed if seed is None else seed, self.lane_offset,
                                              self._t, self._stream())
            _native.check(rc, "pomdp_pick_actions")
        return out

    def heuristic_steps(self, history, steps=1, returns=None):
        """`steps` consecutive steps under the env's own heuristic policy, one launch each
        (pomdp_heuristic_steps): a = choice(_generate_preferred(history)); step(a); side statistics;
        history.append(Transition(observation, a, reward, ob, done)) — the loop of rock.py:557-573 for every lane,
        with the results of that call sequence.  (The reference's own loop builds `Transition(ob, action, next_ob, rw,
        done)` POSITIONALLY into the fields (observation, action, reward, next_observation, done), rock.py:566 — its
        `next_observation` therefore holds the reward and `_generate_preferred`'s history sums never fire there.  This
        path, like the fixtures' harness, fills the fields by name, i.e. the intended order; DESIGN.md §3 lists it among
        the deliberate divergences.)  Returns the last step's (action, ob, reward, done) in reusable
        buffers; `history.prev_ob` holds the observation each lane sees afterwards.  `returns`
        (gym_pomdp_amd.Returns) accumulates the loop's discounted return per lane.  Asynchronous."""
        if not self._has_reset:
            raise AttributeError("%s: heuristic_steps before reset()" % type(self).__name__)
        if history.prev_ob is None:
            raise ValueError("History was built without the current observation: History(env, observation=ob)")
        if self.lane_offset % 4:
            raise ValueError("heuristic_steps: lane_offset must be a multiple of 4 (got %d): the policy's Philox block is shared "
                             "by global lanes 4q .. 4q+3" % self.lane_offset)
        if getattr(self, "_action_scratch", None) is None:
            self._action_scratch = torch.empty(self.batch_size, dtype=torch.int32, device=self.device)
        t0 = self._t
        self._t += int(steps)
        self._dev_flags_used = True
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_heuristic_steps(
                _native.ENV_KIND[self.env_name], self._params_ref, self._state.data_ptr(),
                self._belief_ref() if self.env_name == "rock" else None, history._ref, history.prev_ob.data_ptr(),
                self._action_scratch.data_ptr(), self._ob.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(),
                None if returns is None else returns._ref, self.batch_size, self._seed, self.lane_offset, t0, int(steps),
                _native.POMDP_AUTO_RESET if self.auto_reset else 0, self._stream())
            _native.check(rc, "pomdp_heuristic_steps")
        return self._action_scratch, self._ob, self._reward, self._done.view(torch.bool)

    def collect_heuristic(self, history, steps, layout="packed", out=None, returns=None):
        """heuristic_steps(history, steps) with every step kept (pomdp_heuristic_collect): the same launches leave the env,
        `history`, the side statistics, `returns` and the last step's `_ob / _reward / _done` buffers exactly as
        heuristic_steps does, and row s of the trajectory holds what the policy did at step s — the reference's `history[t]`
        (rock.py:525-550) for every lane: the action it chose, the observation, the reward and done.
        `layout`: "packed" (one 4-byte record per lane-step) or "narrow" (four typed planes per step), as in
        collect_synthetic.  `out`: a dict of trajectory_buffers(k, layout) with k >= steps, reused without allocation; only
        rows 0 .. steps - 1 are written.  Returns that dict: decode_trajectory(out, steps) gives the four columns.
        With auto_reset a done row carries the terminal observation; the observation the fresh episode starts with is NOT
        recorded (history.prev_ob holds it after a launch that ends there).  Without auto_reset a lane whose episode ended
        earlier is frozen: its records are 0x010000FF — action 255 (heuristic_steps reports -1), ob 0, reward 0, done True.
        Asynchronous."""
        if not self._has_reset:
            raise AttributeError("%s: collect_heuristic before reset()" % type(self).__name__)
        if history.prev_ob is None:
            raise ValueError("History was built without the current observation: History(env, observation=ob)")
        if self.lane_offset % 4:
            raise ValueError("collect_heuristic: lane_offset must be a multiple of 4 (got %d): the policy's Philox block is shared "
                             "by global lanes 4q .. 4q+3" % self.lane_offset)
        if layout not in ("packed", "narrow"):
            raise ValueError("collect_heuristic: layout must be 'packed' or 'narrow', got %r" % (layout,))
        steps = int(steps)
        if steps < 0:
            raise ValueError("collect_heuristic: steps must be >= 0")
        if out is None:
            out = self.trajectory_buffers(steps, layout)
        elif out.get("layout") != layout or out["traj"].shape[0] < steps or out["pitch"] < self.batch_size \
                or out["traj"].shape[-1] != out["pitch"] or out["traj"].device != self.device:
            raise ValueError("collect_heuristic: `out` is not a trajectory_buffers(k >= %d, %r) dict of this env" % (steps, layout))
        if steps == 0:
            return out
        if getattr(self, "_action_scratch", None) is None:
            self._action_scratch = torch.empty(self.batch_size, dtype=torch.int32, device=self.device)
        t0 = self._t
        self._t += steps
        self._dev_flags_used = True
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_heuristic_collect(
                _native.ENV_KIND[self.env_name], self._params_ref, self._state.data_ptr(),
                self._belief_ref() if self.env_name == "rock" else None, history._ref, history.prev_ob.data_ptr(),
                self._action_scratch.data_ptr(), self._ob.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(),
                None if returns is None else returns._ref, out["traj"].data_ptr(), int(out["pitch"]), _native.LAYOUTS[layout],
                self.batch_size, self._seed, self.lane_offset, t0, steps,
                _native.POMDP_AUTO_RESET if self.auto_reset else 0, self._stream())
            _native.check(rc, "pomdp_heuristic_collect")
        return out

    def compute_prob(self, action, ob, state=None):
        """`_compute_prob(action, next_state, ob)` per lane -> float64[N]: the likelihood of `ob` given that
        `action` led to `state` (default: the live state)."""
        st = self._state if state is None else self._checked_state(state, None, "compute_prob")
        n = st.shape[1]
        a = torch.as_tensor(action, device=self.device).to(torch.int32).reshape(n).contiguous()
        o = torch.as_tensor(ob, device=self.device).to(torch.int32).reshape(n).contiguous()
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_compute_prob(_native.ENV_KIND[self.env_name], self._params_ref, st.data_ptr(),
                                              a.data_ptr(), o.data_ptr(), out.data_ptr(), n, self._stream())
            _native.check(rc, "pomdp_compute_prob")
        return out

    def _compute_prob(self, action, next_state, ob):
        """Reference signature.  batch_size == 1: python scalars in, float out."""
        if self.batch_size == 1 and not isinstance(action, torch.Tensor):
            return float(self.compute_prob([int(action)], [int(ob)], next_state).item())
        return self.compute_prob(action, ob, next_state)

    def _preferred_policy(self, what, policy, history, all_actions, roots):
        """The checks `policy=` shares between rollout / plan / plan_step -> True when the preferred-policy kernel runs.
        A RockSample env built without use_heuristic answers _generate_preferred with the legal list (rock.py:294-295): its
        preferred rollout IS the uniform one and needs neither history nor side statistics."""
        if policy == "uniform":
            if history is not None:
                raise ValueError("%s: history= goes with policy='preferred'" % what)
            return False
        if policy != "preferred":
            raise ValueError("%s: policy must be 'uniform' or 'preferred', got %r" % (what, policy))
        if all_actions or roots is not None:
            raise ValueError("%s: policy='preferred' excludes all_actions=True and roots=: the side statistics and the history "
                             "describe the live lanes" % what)
        if self.env_name == "rock" and not self._use_heuristic:
            return False
        if history is None or getattr(history, "_env", None) is not self:
            raise ValueError("%s: policy='preferred' needs history=, a gym_pomdp_amd.History of this env" % what)
        if history._max_size is not None:
            raise ValueError("%s: policy='preferred' needs an unbounded History (a simulation would have to carry the window "
                             "of History(max_size=%d))" % (what, history._max_size))
        if self.env_name == "rock" and history.prev_ob is None:
            raise ValueError("History was built without the current observation: History(env, observation=ob)")
        return True

    def _preferred_args(self, history, n_sims, out):
        """(belief, history, prev_ob, workspace) of pomdp_rollout_preferred; the workspace is cached in `out`"""
        if self.env_name != "rock":
            return None, history._ref, None, None
        ws = out.get("_workspace")
        nbytes = 32 * self.num_rocks * n_sims
        if ws is None or ws.numel() != nbytes:
            ws = out["_workspace"] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._belief_ref(), history._ref, history.prev_ob.data_ptr(), ws.data_ptr()

    def rollout(self, depth, sims_per_root=1, roots=None, discount=None, all_actions=False, lane_offset=None, out=None,
                policy="uniform", history=None):
        """Random rollouts from `roots` (packed states int32 [state_words, R]; default: the live state):
        R * sims_per_root independent simulations of at most `depth` steps under a uniform policy over
        `_generate_legal()` (or over all actions), discounted by `discount` (default: the env's
        `_discount`).  Neither `roots` nor the live state is modified; the call counter advances by
        `depth`.  Returns a dict of per-simulation tensors: ret float64, n_steps, first_action, last_ob
        int32, terminated bool — simulation i belongs to root i // sims_per_root.  `out`: the dict of an earlier
        call of the same shape, to reuse its buffers.
        `policy="preferred"` with `history=` (an unbounded History of this env): every simulation picks from
        `_generate_preferred(history)` instead — the env's own rollout policy, as POMCP uses it — starting from the live
        lanes' side statistics and history and keeping its own copies of them as it goes (pomdp_rollout_preferred)."""
        preferred = self._preferred_policy("rollout", policy, history, all_actions, roots)
        st = self._state if roots is None else self._checked_state(roots, None, "rollout")
        n_roots = st.shape[1]
        n = n_roots * int(sims_per_root)
        if (self.lane_offset if lane_offset is None else int(lane_offset)) % 4:
            raise ValueError("rollout: the simulations' first global lane must be a multiple of 4 (quad-shared Philox blocks)")
        t0 = self._t
        self._t += int(depth)
        if out is None:
            out = dict(ret=torch.empty(n, dtype=torch.float64, device=self.device),
                       n_steps=torch.empty(n, dtype=torch.int32, device=self.device),
                       first_action=torch.empty(n, dtype=torch.int32, device=self.device),
                       last_ob=torch.empty(n, dtype=torch.int32, device=self.device),
                       terminated=torch.empty(n, dtype=torch.uint8, device=self.device))
        else:                              # a dict returned by an earlier call of the same shape: buffers are reused
            out["terminated"] = out["terminated"].view(torch.uint8)
        if preferred:
            with torch.cuda.device(self.device):
                rc = self._lib.pomdp_rollout_preferred(
                    _native.ENV_KIND[self.env_name], self._params_ref, st.data_ptr(), n_roots, 1, int(sims_per_root), int(depth),
                    float(self._discount if discount is None else discount), *self._preferred_args(history, n, out), self._seed,
                    self.lane_offset if lane_offset is None else int(lane_offset), t0, out["ret"].data_ptr(),
                    out["n_steps"].data_ptr(), out["first_action"].data_ptr(), out["last_ob"].data_ptr(),
                    out["terminated"].data_ptr(), self._stream())
                _native.check(rc, "pomdp_rollout_preferred")
            out["terminated"] = out["terminated"].view(torch.bool)
            return out
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_rollout(
                _native.ENV_KIND[self.env_name], self._params_ref, st.data_ptr(), n_roots, int(sims_per_root),
                int(depth), float(self._discount if discount is None else discount),
                _native.POMDP_ROLLOUT_ALL_ACTIONS if all_actions else 0, self._seed,
                self.lane_offset if lane_offset is None else int(lane_offset), t0, out["ret"].data_ptr(),
                out["n_steps"].data_ptr(), out["first_action"].data_ptr(), out["last_ob"].data_ptr(),
                out["terminated"].data_ptr(), self._stream())
            _native.check(rc, "pomdp_rollout")
        out["terminated"] = out["terminated"].view(torch.bool)
        return out

    def plan(self, depth, sims_per_root=1024, discount=None, all_actions=False, roots=None, out=None, belief=None,
             policy="uniform", history=None):
        """One planning pass of a POMCP-style caller over the live state (or `roots`): `sims_per_root` random rollouts of
        at most `depth` steps from every root (rollout()), reduced ON THE DEVICE to the roots' action values
        (pomdp_plan): {"q": float64 [R, n_actions] mean return by first action (0 where never tried), "visits": int32
        [R, n_actions], "best": int32 [R] the visited action with the largest q (lowest index on ties, -1 if no
        simulation took a step), "value": float64 [R] = q[best], "sim_ret" / "sim_first_action": the R * sims_per_root
        simulations' returns and first actions}.  The float64 sums follow the order stated in include/pomdp_hip.h, so the
        CPU restatement reproduces them bit for bit.  Root r is global lane lane_offset + r and its simulation s is
        global lane (lane_offset + r) * sims_per_root + s: the draws — and with them q / visits / best — do not depend on
        how the roots are sharded, and whole roots never straddle a shard.  The call counter advances by `depth`.
        `out`: the dict of an earlier call of the same shape, to reuse its buffers.  Asynchronous.
        Without `belief` the roots are the TRUE states: flat Monte Carlo with the hidden state known.  `belief` (a
        ParticleBelief of this env, particle_belief()): plan from its particles instead (pomdp_plan_particles) — particle p of
        root r runs sims_per_root / P of the root's simulations (simulation p * (sims_per_root / P) + s, the same global lanes
        as above); sims_per_root must be a multiple of P.
        `policy="preferred"` with `history=` (an unbounded History of this env): the simulations roll out under
        `_generate_preferred(history)` as in rollout() (pomdp_plan_preferred), from the true states or from `belief`'s
        particles; the side statistics and the history are the live lanes' either way."""
        preferred = self._preferred_policy("plan", policy, history, all_actions, roots)
        if belief is not None:
            if roots is not None:
                raise ValueError("plan: roots= and belief= exclude each other")
            if not belief._shape_ok(self):
                raise ValueError("plan: the belief belongs to another env shape (%r)" % (belief,))
            if int(sims_per_root) % belief.n_particles:
                raise ValueError("plan: sims_per_root (%d) must be a multiple of the belief's particle count (%d)"
                                 % (int(sims_per_root), belief.n_particles))
        st = self._state if roots is None else self._checked_state(roots, None, "plan")
        n_roots, sims, depth = st.shape[1], int(sims_per_root), int(depth)
        n, n_act = n_roots * sims, self.action_space.n
        sim_lane0 = self.lane_offset * sims
        if sims < 1 or sim_lane0 + n > 1 << 32:
            raise ValueError("plan: the simulations' global lanes (lane_offset + r) * sims_per_root + s must lie in [0, 2^32)")
        if sim_lane0 % 4:
            raise ValueError("plan: lane_offset * sims_per_root must be a multiple of 4 (quad-shared Philox blocks)")
        if out is None:
            out = dict(q=torch.zeros((n_roots, n_act), dtype=torch.float64, device=self.device),
                       visits=torch.zeros((n_roots, n_act), dtype=torch.int32, device=self.device),
                       best=torch.empty(n_roots, dtype=torch.int32, device=self.device),
                       value=torch.empty(n_roots, dtype=torch.float64, device=self.device),
                       sim_ret=torch.empty(n, dtype=torch.float64, device=self.device),
                       sim_first_action=torch.empty(n, dtype=torch.int32, device=self.device))
        elif out["q"].shape != (n_roots, n_act) or out["sim_ret"].shape != (n,):
            raise ValueError("plan: `out` was built for another shape")
        po = out.get("_plan_out")
        if po is None:
            po = out["_plan_out"] = _native.PlanOut(q=out["q"].data_ptr(), visits=out["visits"].data_ptr(), best=out["best"].data_ptr(),
                                                    value=out["value"].data_ptr(), stride=n_act, reserved=0)
        t0 = self._t
        self._t += depth
        if preferred:
            with torch.cuda.device(self.device):
                rc = self._lib.pomdp_plan_preferred(
                    _native.ENV_KIND[self.env_name], self._params_ref,
                    st.data_ptr() if belief is None else belief.particles.data_ptr(), n_roots,
                    1 if belief is None else belief.n_particles, sims, depth,
                    float(self._discount if discount is None else discount), *self._preferred_args(history, n, out), self._seed,
                    sim_lane0, t0, out["sim_ret"].data_ptr(), out["sim_first_action"].data_ptr(), C.byref(po), self._stream())
                _native.check(rc, "pomdp_plan_preferred")
            return out
        with torch.cuda.device(self.device):
            if belief is not None:
                rc = self._lib.pomdp_plan_particles(
                    _native.ENV_KIND[self.env_name], self._params_ref, belief.particles.data_ptr(), n_roots, belief.n_particles,
                    sims, depth, float(self._discount if discount is None else discount),
                    _native.POMDP_ROLLOUT_ALL_ACTIONS if all_actions else 0, self._seed, sim_lane0, t0, out["sim_ret"].data_ptr(),
                    out["sim_first_action"].data_ptr(), C.byref(po), self._stream())
                _native.check(rc, "pomdp_plan_particles")
                return out
            rc = self._lib.pomdp_plan(
                _native.ENV_KIND[self.env_name], self._params_ref, st.data_ptr(), n_roots, sims, depth,
                float(self._discount if discount is None else discount), _native.POMDP_ROLLOUT_ALL_ACTIONS if all_actions else 0,
                self._seed, sim_lane0, t0, out["sim_ret"].data_ptr(), out["sim_first_action"].data_ptr(), C.byref(po), self._stream())
            _native.check(rc, "pomdp_plan")
        return out

    def plan_step(self, depth, sims_per_root=1024, discount=None, all_actions=False, out=None, belief=None,
                  policy="uniform", history=None):
        """One REAL step of every lane, planned: plan() from the live state, then step(best) — BASELINE.json configs[4]'s "1024-
        simulation rollout per real step".  Returns (ob, reward, done, info, plan dict).  A lane whose simulations took no
        step (best == -1: nothing legal to do, or depth == 0) is handed -1, which step() counts as an invalid action and
        leaves untouched.  batch_size == 1: python scalars as step() returns them.
        `belief` (a ParticleBelief of this env): plan from its particles, step(best), then belief.update(best, ob, reward,
        done) — the belief follows what the real step showed.  Needs auto_reset=False (an auto-reset step would not deliver
        the fresh episode's observation).  Ended lanes are restarted by the caller, env and belief together:
            ob = env.reset(where=done); belief.reset(ob, where=done)
        `policy="preferred"` with `history=`: plan under the env's preferred-action policy, then keep the agent's knowledge in
        step with the real step: step() updates RockSample's side statistics (pomdp_rock_belief_update), the transition
        (history.prev_ob, best, reward, ob, done) is appended to `history` (pomdp_history_append) and history.prev_ob becomes
        ob — next to belief.update(...) when `belief` is given.  Needs auto_reset=False for the same reason; the caller
        restarts ended lanes with env.reset(where=done), belief.reset(ob, where=done), history.clear(where=done) and
        history.prev_ob[done] = ob[done]."""
        if belief is not None and self._auto_reset:
            raise ValueError("plan_step(belief=...) needs auto_reset=False: restart ended lanes with env.reset(where=done) and "
                             "belief.reset(ob, where=done)")
        if policy == "preferred" and self._auto_reset:
            raise ValueError("plan_step(policy='preferred') needs auto_reset=False: restart ended lanes with env.reset(where=done) "
                             "and history.clear(where=done)")
        p = self.plan(depth, sims_per_root, discount, all_actions, out=out, belief=belief, policy=policy, history=history)
        a = p["best"]
        if self.batch_size == 1:
            a = int(a.item())
            assert a >= 0, "plan_step: no simulation took a step"
        res = self.step(a)
        if history is not None:
            from ..history import Transition
            history.append(Transition(history.prev_ob, a, res[1], res[0], res[2]), auto_reset=False)
            if history.prev_ob is not None:
                history.prev_ob.copy_(torch.as_tensor(res[0], device=self.device).to(torch.int32).reshape(self.batch_size))
        if belief is not None:
            belief.update(a, res[0], res[1], res[2])
        return res + (p,)

    def search(self, depth, sims_per_tree, trees_per_root, ucb_c, discount=None, belief=None, out=None, diagnostics=False,
               policy="uniform", history=None, prior_n=0, prior_v=0.0, tree=None):
        """POMCP's tree search from the live state (pomdp_tree_search): for every lane `trees_per_root` independent UCB1 trees
        over action-observation histories, each grown by `sims_per_tree` simulations of at most `depth` steps — UCB1 with
        exploration constant `ucb_c` inside the tree, one new node per simulation, a uniform random rollout over
        `_generate_legal()` from the new leaf — merged per root ON THE DEVICE.  Returns plan()'s keys {"q", "visits", "best",
        "value"} ([R, n_actions] / [R]: visits summed and values visit-weighted over the root's trees) plus the trees' own
        root statistics "tree_visits" int32 / "tree_q" float64 [R * trees_per_root, n_actions] and "n_nodes" int32
        [R * trees_per_root]; `diagnostics=True` adds per-simulation "sim_ret" float64, "sim_steps" and "sim_tree_steps"
        int32, each [sims_per_tree, R * trees_per_root].  Every float64 operation and its order are stated in
        include/pomdp_hip.h, so the CPU restatement reproduces the result bit for bit.  Tree w of root r is global lane
        (lane_offset + r) * trees_per_root + w: nothing depends on how the roots are sharded.  The call counter advances by
        sims_per_tree * depth.  `ucb_c` has no default: the reference ships no planner to copy one from, and the right value
        scales with the env's returns.
        Without `belief` the simulations start from the TRUE states; `belief` (a ParticleBelief of this env): every
        simulation starts from a particle of its root drawn anew (stream TREE).  `out`: the dict of an earlier call of the same
        shape, to reuse its buffers, the workspaces and the log table.  Asynchronous.
        `policy="preferred"` with `history=` (an unbounded History of this env): POMCP as it runs on RockSample and Tag
        (pomdp_tree_search_preferred).  Every simulation starts from the live lanes' side statistics and history, keeps its own
        copies of them through the tree and the rollout, and rolls out under `_generate_preferred(history)`; nothing of the
        env or the History is written.  `prior_n` > 0 (at most 65535) with `prior_v`: a new node's preferred actions start with
        N = prior_n and V = prior_v ("smart tree"), and "tree_visits" / "visits" include those counts.  The envs whose
        preferred list is the legal list, and a RockSample env built without use_heuristic, run the uniform search; with
        prior_n > 0 they raise ValueError: a uniform prior over the legal list steers nothing.
        `tree` (a SearchTree of this env, trees_per_root and depth: env.search_tree(...)): the uniform search resumed from the
        nodes `tree` holds (pomdp_tree_search_resume) — empty trees at first, after tree.advance(action, ob) the subtrees under
        the real step.  "tree_visits" / "visits" then include the kept visits, "n_nodes" are the trees' sizes afterwards (also
        tree.n_nodes), and a tree that has filled its node_capacity keeps simulating without growing.  A tree is bound to the
        policy it is grown under: on RockSample with use_heuristic=True and on Tag, policy="preferred" resumes only a tree
        built with search_tree(..., policy="preferred", prior_n=, prior_v=) (pomdp_tree_search_preferred_resume) and takes its
        priors from the tree — prior_n / prior_v that differ from the tree's raise ValueError, the defaults mean "the
        tree's" —, a kept node is primed once, by the first simulation that stands on it while its Nh is 0; a default tree
        under policy="preferred", and a preferred tree under policy="uniform", raise ValueError."""
        import math
        preferred = self._preferred_policy("search", policy, history, False, None)
        prior_n, prior_v = int(prior_n), float(prior_v)
        if prior_n < 0 or prior_n > 65535 or not math.isfinite(prior_v):
            raise ValueError("search: needs 0 <= prior_n <= 65535 and a finite prior_v, got %r, %r" % (prior_n, prior_v))
        preferred = preferred and self.env_name in ("rock", "tag")
        if prior_n > 0 and not preferred:
            raise ValueError("search: prior_n > 0 needs policy='preferred' on an env with a preferred-action policy of its own "
                             "(RockSample with use_heuristic=True, Tag): a uniform prior over the legal list steers nothing")
        if belief is not None and not belief._shape_ok(self):
            raise ValueError("search: the belief belongs to another env shape (%r)" % (belief,))
        R, n_act = self._state.shape[1], self.action_space.n
        D, S, W = int(depth), int(sims_per_tree), int(trees_per_root)
        if tree is not None:
            if preferred and tree.policy != "preferred":
                raise ValueError("search: the preferred-policy search does not resume a tree grown without priors: tree= needs "
                                 "policy='uniform' on this env, or build the tree with search_tree(..., policy='preferred')")
            if not preferred and tree.policy == "preferred":
                raise ValueError("search: a SearchTree built with policy='preferred' is resumed by search(policy='preferred', "
                                 "history=...) only: its nodes carry priors the uniform search does not lay")
            if preferred:
                if (prior_n, prior_v) != (0, 0.0) and (prior_n, prior_v) != (tree.prior_n, tree.prior_v):
                    raise ValueError("search: prior_n=%r, prior_v=%r differ from the SearchTree's (%r, %r): with tree= the priors "
                                     "are the tree's" % (prior_n, prior_v, tree.prior_n, tree.prior_v))
                prior_n, prior_v = tree.prior_n, tree.prior_v
            if not tree._belongs(self, W, D):
                raise ValueError("search: the SearchTree belongs to another env shape, trees_per_root or depth")
        n = R * W
        lane0 = self.lane_offset * W
        if W < 1 or S < 1 or D < 0 or lane0 + n > 1 << 32:
            raise ValueError("search: needs trees_per_root >= 1, sims_per_tree >= 1, depth >= 0 and the trees' global lanes "
                             "(lane_offset + r) * trees_per_root + w in [0, 2^32)")
        if lane0 % 4:
            raise ValueError("search: lane_offset * trees_per_root must be a multiple of 4 (quad-shared Philox blocks)")
        c = float(ucb_c)
        if not (c >= 0.0 and math.isfinite(c)):
            raise ValueError("search: ucb_c must be finite and >= 0, got %r" % (ucb_c,))
        kind = _native.ENV_KIND[self.env_name]
        if out is None:
            dev = self.device
            out = dict(q=torch.zeros((R, n_act), dtype=torch.float64, device=dev),
                       visits=torch.zeros((R, n_act), dtype=torch.int32, device=dev),
                       best=torch.empty(R, dtype=torch.int32, device=dev), value=torch.empty(R, dtype=torch.float64, device=dev),
                       tree_visits=torch.zeros((n, n_act), dtype=torch.int32, device=dev),
                       tree_q=torch.zeros((n, n_act), dtype=torch.float64, device=dev),
                       n_nodes=torch.empty(n, dtype=torch.int32, device=dev))
        elif out["q"].shape != (R, n_act) or out["tree_q"].shape != (n, n_act):
            raise ValueError("search: `out` was built for another shape")
        if diagnostics and ("sim_ret" not in out or out["sim_ret"].shape != (S, n)):
            out["sim_ret"] = torch.empty((S, n), dtype=torch.float64, device=self.device)
            out["sim_steps"] = torch.empty((S, n), dtype=torch.int32, device=self.device)
            out["sim_tree_steps"] = torch.empty((S, n), dtype=torch.int32, device=self.device)
        if tree is not None:
            return self._search_resume(tree, out, belief, diagnostics, R, W, S, D, c, discount, lane0, n_act,
                                       history if preferred else None)
        nbytes = int(self._lib.pomdp_tree_search_workspace(kind, self._params_ref, n, S, D))
        if nbytes == 0 and n > 0:
            raise ValueError("search: pomdp_tree_search_workspace refuses %d trees x %d simulations x depth %d" % (n, S, D))
        ws = out.get("_workspace")
        if ws is None or ws.numel() * 8 != nbytes:
            ws = out["_workspace"] = torch.empty((nbytes // 16, 2), dtype=torch.float64, device=self.device)   # 16-byte units
        n_log = S + 1 + n_act * prior_n                      # Nh counts the priors
        if prior_n > 0 and W * (n_log - 1) > 0x7FFFFFFF:
            raise ValueError("search: trees_per_root * (sims_per_tree + n_actions * prior_n) must stay below 2^31 (merged visits)")
        logn = out.get("_logn")
        if logn is None or logn.numel() != n_log:
            logn = out["_logn"] = torch.tensor([float("-inf")] + [math.log(k) for k in range(1, n_log)], dtype=torch.float64).to(self.device)
        diag = lambda k: out[k].data_ptr() if diagnostics else None
        args = _native.PlanTreeArgs(
            env=kind, depth=D, params=C.addressof(self._params), root_state=self._state.data_ptr(),
            particles=None if belief is None else belief.particles.data_ptr(), n_roots=R,
            n_particles=0 if belief is None else belief.n_particles, trees_per_root=W, sims_per_tree=S,
            discount=float(self._discount if discount is None else discount), ucb_c=c, logn=logn.data_ptr(),
            workspace=ws.data_ptr(), workspace_bytes=nbytes, tree_visits=out["tree_visits"].data_ptr(),
            tree_q=out["tree_q"].data_ptr(), n_nodes=out["n_nodes"].data_ptr(), sim_ret=diag("sim_ret"),
            sim_steps=diag("sim_steps"), sim_tree_steps=diag("sim_tree_steps"),
            out=_native.PlanOut(q=out["q"].data_ptr(), visits=out["visits"].data_ptr(), best=out["best"].data_ptr(),
                                value=out["value"].data_ptr(), stride=n_act, reserved=0),
            seed=self._seed, lane0=lane0, reserved=0)
        t0 = self._t
        self._t += S * D
        if preferred:
            rock = self.env_name == "rock"
            pbytes = int(self._lib.pomdp_tree_search_preferred_workspace(kind, self._params_ref, n))
            pws = out.get("_policy_workspace")
            if pws is None or pws.numel() * 8 != pbytes:
                pws = out["_policy_workspace"] = torch.empty((pbytes // 16, 2), dtype=torch.float64, device=self.device)
            pol = _native.PlanTreePolicy(
                belief=C.addressof(self._tracker.ptrs) if rock else None, history=C.addressof(history._ptrs),
                prev_ob=history.prev_ob.data_ptr() if rock else None, workspace=pws.data_ptr() if pbytes else None,
                workspace_bytes=pbytes, prior_n=prior_n, reserved=0, prior_v=prior_v)
            with torch.cuda.device(self.device):
                rc = self._lib.pomdp_tree_search_preferred(C.byref(args), C.byref(pol), t0, self._stream())
                _native.check(rc, "pomdp_tree_search_preferred")
            return out
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_tree_search(C.byref(args), t0, self._stream())
            _native.check(rc, "pomdp_tree_search")
        return out

    def _search_resume(self, tree, out, belief, diagnostics, R, W, S, D, c, discount, lane0, n_act, history=None):
        """search(tree=...) after its checks: pomdp_tree_search_resume — with `history` (a preferred tree)
        pomdp_tree_search_preferred_resume under the tree's priors — into the buffers of `out`"""
        logn, keep = tree._begin_search(S)
        diag = lambda k: out[k].data_ptr() if diagnostics else None
        args = _native.PlanTreeArgs(
            env=_native.ENV_KIND[self.env_name], depth=D, params=C.addressof(self._params), root_state=self._state.data_ptr(),
            particles=None if belief is None else belief.particles.data_ptr(), n_roots=R,
            n_particles=0 if belief is None else belief.n_particles, trees_per_root=W, sims_per_tree=S,
            discount=float(self._discount if discount is None else discount), ucb_c=c, logn=logn.data_ptr(),
            workspace=None, workspace_bytes=0, tree_visits=out["tree_visits"].data_ptr(),
            tree_q=out["tree_q"].data_ptr(), n_nodes=out["n_nodes"].data_ptr(), sim_ret=diag("sim_ret"),
            sim_steps=diag("sim_steps"), sim_tree_steps=diag("sim_tree_steps"),
            out=_native.PlanOut(q=out["q"].data_ptr(), visits=out["visits"].data_ptr(), best=out["best"].data_ptr(),
                                value=out["value"].data_ptr(), stride=n_act, reserved=0),
            seed=self._seed, lane0=lane0, reserved=0)
        t0 = self._t
        self._t += S * D
        if history is not None:
            rock = self.env_name == "rock"
            pbytes = int(self._lib.pomdp_tree_search_preferred_workspace(args.env, self._params_ref, R * W))
            pws = tree._policy_workspace                     # scratch, uninitialised between calls: held by the tree
            if pws is None or pws.numel() * 8 != pbytes:
                pws = tree._policy_workspace = torch.empty((pbytes // 16, 2), dtype=torch.float64, device=self.device)
            pol = _native.PlanTreePolicy(
                belief=C.addressof(self._tracker.ptrs) if rock else None, history=C.addressof(history._ptrs),
                prev_ob=history.prev_ob.data_ptr() if rock else None, workspace=pws.data_ptr() if pbytes else None,
                workspace_bytes=pbytes, prior_n=tree.prior_n, reserved=0, prior_v=tree.prior_v)
            with torch.cuda.device(self.device):
                rc = self._lib.pomdp_tree_search_preferred_resume(C.byref(args), C.byref(pol), C.byref(keep), t0, self._stream())
                _native.check(rc, "pomdp_tree_search_preferred_resume")
            return out
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_tree_search_resume(C.byref(args), C.byref(keep), t0, self._stream())
            _native.check(rc, "pomdp_tree_search_resume")
        return out

    def search_tree(self, trees_per_root, node_capacity=None, depth=64, sims_per_tree=None, policy="uniform", prior_n=0,
                    prior_v=0.0):
        """A SearchTree for search(tree=...) / search_step(tree=...) of this env: `trees_per_root` trees per lane, each a pool of
        `node_capacity` nodes (None with `sims_per_tree=`: 2 * sims_per_tree + 1), for searches of this `depth`.
        `policy` binds the tree to the search that grows it: "uniform" (the default), or "preferred" with the node priors
        `prior_n` / `prior_v` for search(policy="preferred", history=..., tree=tree) on RockSample with use_heuristic=True and
        on Tag.  On the envs whose preferred search is the uniform one, "preferred" with prior_n == 0 gives a uniform tree and
        prior_n > 0 raises ValueError, as search() does."""
        from ..search_tree import SearchTree
        return SearchTree(self, trees_per_root, node_capacity, depth, sims_per_tree, policy, prior_n, prior_v)

    def search_step(self, depth, sims_per_tree, trees_per_root, ucb_c, discount=None, belief=None, out=None, diagnostics=False,
                    policy="uniform", history=None, prior_n=0, prior_v=0.0, tree=None):
        """One REAL step of every lane, searched: search() from the live state (or from `belief`'s particles), then step(best)
        and, with `belief`, belief.update(best, ob, reward, done) — what plan_step() is to plan().  Returns (ob, reward, done,
        info, search dict).  A lane whose search took no step (best == -1) is handed -1, which step() counts as an invalid
        action.  With `belief` it needs auto_reset=False; the caller restarts ended lanes as after plan_step().
        `policy="preferred"` with `history=` (and `prior_n`, `prior_v`): search() under the env's preferred-action policy, then
        the agent's knowledge follows the real step exactly as in plan_step(): step() updates RockSample's side statistics, the
        transition (history.prev_ob, best, reward, ob, done) is appended to `history` and history.prev_ob becomes ob — next to
        belief.update(...) when `belief` is given.  Needs auto_reset=False for the same reason.
        `tree` (search()): the search resumes from `tree`, and after the real step tree.advance(best, ob, drop=done) keeps the
        subtrees under it: the trees of ended lanes and of lanes with best == -1 end up empty.  Needs auto_reset=False: a
        restarted lane's tree would be the old episode's."""
        if tree is not None and self._auto_reset:
            raise ValueError("search_step(tree=...) needs auto_reset=False: restart ended lanes with env.reset(where=done); "
                             "their trees are already empty")
        if belief is not None and self._auto_reset:
            raise ValueError("search_step(belief=...) needs auto_reset=False: restart ended lanes with env.reset(where=done) and "
                             "belief.reset(ob, where=done)")
        if policy == "preferred" and self._auto_reset:
            raise ValueError("search_step(policy='preferred') needs auto_reset=False: restart ended lanes with "
                             "env.reset(where=done) and history.clear(where=done)")
        p = self.search(depth, sims_per_tree, trees_per_root, ucb_c, discount, belief=belief, out=out, diagnostics=diagnostics,
                        policy=policy, history=history, prior_n=prior_n, prior_v=prior_v, tree=tree)
        a = p["best"]
        if self.batch_size == 1:
            a = int(a.item())
            assert a >= 0, "search_step: no simulation took a step"
        res = self.step(a)
        if tree is not None:
            tree.advance(p["best"], res[0], drop=res[2])
        if history is not None:
            from ..history import Transition
            history.append(Transition(history.prev_ob, a, res[1], res[0], res[2]), auto_reset=False)
            if history.prev_ob is not None:
                history.prev_ob.copy_(torch.as_tensor(res[0], device=self.device).to(torch.int32).reshape(self.batch_size))
        if belief is not None:
            belief.update(a, res[0], res[1], res[2])
        return res + (p,)

    def particle_belief(self, n_particles=256, seed=None):
        """A ParticleBelief of n_particles particles per lane of this env (gym_pomdp_amd.particles); call its reset(ob) with
        the observation of this env's reset() before planning from it."""
        from ..particles import ParticleBelief
        return ParticleBelief(self, n_particles, seed)

    def rollout_synthetic(self, steps, action_seed=None, actions=None, fuse=False):
        """`steps` consecutive step() calls under the synthetic uniform policy, issued from C
        (pomdp_rollout_synthetic): the same launches per step a python loop over synthetic_actions() + step()
        makes, without the interpreter between them.  `fuse=True` (policy key == env key only): up to pomdp_fuse_max()
        (256) consecutive steps share one launch — every step's outputs are still computed and written, so all
        buffers end up exactly as after the per-step launches, but a lane's state stays in registers between
        its steps.  Outputs land in the reusable buffers; returns (ob, reward, done) of the last step.
        Asynchronous."""
        if not self._has_reset:
            raise AttributeError("%s: rollout before reset()" % type(self).__name__)
        self._check_driver_use("rollout_synthetic")
        if actions is None:
            if getattr(self, "_action_scratch", None) is None:
                self._action_scratch = torch.empty(self.batch_size, dtype=torch.int32, device=self.device)
            actions = self._action_scratch
        t0 = self._t
        self._t += int(steps)
        self._dev_flags_used = True
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_rollout_synthetic(
                _native.ENV_KIND[self.env_name], self._params_ref, self._state.data_ptr(), actions.data_ptr(),
                self._ob.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(), self._err.data_ptr(),
                self.batch_size, self._seed, self._seed if action_seed is None else action_seed, self.lane_offset,
                t0, int(steps), (_native.POMDP_AUTO_RESET if self.auto_reset else 0) |
                (_native.POMDP_FUSE_STEPS if fuse else 0), self._stream())
            _native.check(rc, "pomdp_rollout_synthetic")
        return self._ob, self._reward, self._done.view(torch.bool)

    def trajectory_buffers(self, steps, layout="columns"):
        """The `out` dict of collect_synthetic(steps, layout=...).
        "columns" (the default ABI): action int32 [steps + 1, N], ob int32 [steps, N], reward [steps, N], done bool
        [steps, N] (and its uint8 view "done_u8"), carved from one allocation with staggered column starts.
        "blocked" / "packed" / "narrow" (include/pomdp_hip.h: POMDP_LAYOUT_*; one write stream per step): {"layout", "traj":
        the raw rows — uint8 [steps, pitch * 13] / int32 [steps, pitch] / uint8 [steps, 4, pitch] —, "pitch"};
        decode_trajectory() gives the four columns (narrow: its typed planes, in place)."""
        n = self.batch_size
        if layout == "columns":
            a, o, r, d = staggered([((steps + 1, n), torch.int32), ((steps, n), torch.int32), ((steps, n), self._reward.dtype),
                                    ((steps, n), torch.uint8)], self.device)
            return {"action": a, "ob": o, "reward": r, "done_u8": d, "done": d.view(torch.bool)}       # no "layout" key = columns
        if layout == "blocked":
            pitch = -(-n // 256) * 256
            return {"layout": "blocked", "pitch": pitch, "traj": torch.zeros((steps, pitch * 13), dtype=torch.uint8, device=self.device)}
        if layout == "packed":
            pitch = -(-n // 4) * 4
            return {"layout": "packed", "pitch": pitch, "traj": torch.zeros((steps, pitch), dtype=torch.int32, device=self.device)}
        if layout == "narrow":
            pitch = -(-n // 16) * 16
            return {"layout": "narrow", "pitch": pitch, "traj": torch.zeros((steps, 4, pitch), dtype=torch.uint8, device=self.device)}
        raise ValueError("unknown trajectory layout %r (columns, blocked, packed, narrow)" % (layout,))

    def packed_reward_table(self):
        """reward_code byte of a packed record -> the reward the columns hold (pomdp_packed_reward), as a [256] tensor of
        this env's reward dtype."""
        t = getattr(self, "_packed_reward_table", None)
        if t is None:
            kind = _native.ENV_KIND[self.env_name]
            vals = [self._lib.pomdp_packed_reward(kind, c) for c in range(256)]
            t = self._packed_reward_table = torch.tensor(vals, dtype=torch.float64).to(self._reward.dtype).to(self.device)
        return t

    def decode_trajectory(self, out, steps=None, into=None):
        """The four columns of a collected trajectory whatever its layout: {"action" (the action taken at each step), "ob",
        "reward", "done"}, each [steps, N].
        columns: the buffers themselves.  blocked: int32 / reward-dtype / bool COPIES gathered from the 256-lane blocks.
        packed: int32 / reward-dtype / bool columns written by ONE device pass over the records (pomdp_decode_packed: 4 bytes
        read, 13 written per lane-step) — into `into` (a trajectory_buffers(steps) dict; rows 0 .. steps - 1 of its
        "action") when given.  narrow: the planes themselves, no copy — action / ob uint8, done bool, reward int8 (the
        reward itself; Network: its values through packed_reward_table(), a gather)."""
        layout = out.get("layout", "columns")
        n = self.batch_size
        if layout == "columns":
            k = out["ob"].shape[0] if steps is None else steps
            return {"action": out["action"][:k], "ob": out["ob"][:k], "reward": out["reward"][:k], "done": out["done"][:k]}
        traj = out["traj"] if steps is None else out["traj"][:steps]
        k = traj.shape[0]
        if layout == "blocked":
            b = traj.view(k, out["pitch"] // 256, 13 * 256)
            col = lambda lo, dt: b[:, :, lo:lo + 1024].view(dt).reshape(k, -1)[:, :n]                     # noqa: E731
            return {"action": col(0, torch.int32), "ob": col(1024, torch.int32), "reward": col(2048, self._reward.dtype),
                    "done": b[:, :, 3072:].reshape(k, -1)[:, :n].view(torch.bool)}
        if layout == "narrow":
            rw = traj[:, 2, :n]
            rw = self.packed_reward_table()[rw.long()] if self.env_name == "network" else rw.view(torch.int8)
            return {"action": traj[:, 0, :n], "ob": traj[:, 1, :n], "reward": rw, "done": traj[:, 3, :n].view(torch.bool)}
        if into is None:
            into = self.trajectory_buffers(k)
        if into["ob"].shape[0] < k or into["ob"].shape[1] != n:
            raise ValueError("decode_trajectory: `into` does not have the shapes of trajectory_buffers(%d)" % k)
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_decode_packed(_native.ENV_KIND[self.env_name], traj.data_ptr(), n, k, int(out["pitch"]),
                                               into["action"].data_ptr(), into["ob"].data_ptr(), into["reward"].data_ptr(),
                                               into["done_u8"].data_ptr(), n, self._stream())
            _native.check(rc, "pomdp_decode_packed")
        return {"action": into["action"][:k], "ob": into["ob"][:k], "reward": into["reward"][:k], "done": into["done"][:k]}

    def collect_returns(self, steps, stats=None, discount=None):
        """`steps` consecutive step() calls under the synthetic uniform policy with NOTHING kept per step but the reduction
        the reference's callers apply to the stream (pomdp_collect_returns): per lane `r += discount * rw; discount *=
        _discount`, the return of every finished episode banked (network.py:175-191, rock.py:553-575).  Same policy, same
        draws and same final state as collect_synthetic(steps).  `stats`: a gym_pomdp_amd.EpisodeStats to continue
        (default: a fresh one with the env's `_discount`).  Returns it.  Asynchronous."""
        if not self._has_reset:
            raise AttributeError("%s: collect before reset()" % type(self).__name__)
        if not self.auto_reset:
            raise ValueError("collect_returns needs auto_reset=True")
        self._check_driver_use("collect_returns")
        if stats is None:
            from ..history import EpisodeStats
            stats = EpisodeStats(self, discount)
        elif stats._n != self.batch_size or stats.acc.device != self.device:
            raise ValueError("collect_returns: `stats` belongs to another batch")
        steps = int(steps)
        t0 = self._t
        self._t = t0 + steps
        with torch.cuda.device(self.device):
            rc = self._lib.pomdp_collect_returns(_native.ENV_KIND[self.env_name], self._params_ref, self._ptrs[0], stats._ref,
                                                 self._ptrs[4], self.batch_size, self._seed, self.lane_offset, t0, steps,
                                                 _native.POMDP_AUTO_RESET, self._stream())
            _native.check(rc, "pomdp_collect_returns")
        return stats

    def as_tape(self, actions):
        """`actions` ([steps, N], any integer dtype, any device) as the uint8 tape the fused launches read: a uint8 tensor on
        this env's device whose rows are contiguous is used in place (e.g. the action plane `traj["traj"][:, 0]` of a narrow
        trajectory); anything else is converted, an action that does not fit a byte becoming 255 (out of range for every env,
        so it stays the invalid action it was)."""
        if (isinstance(actions, torch.Tensor) and actions.dtype == torch.uint8 and actions.device == self.device and actions.dim() == 2
                and actions.shape[1] == self.batch_size and actions.stride(1) == 1
                and (actions.shape[0] <= 1 or actions.stride(0) >= actions.shape[1])):
            return actions                                    # already a tape: the common case costs one test
        t = torch.as_tensor(actions, device=self.device) if not isinstance(actions, torch.Tensor) else actions.to(self.device)
        if t.dim() != 2 or t.shape[1] != self.batch_size:
            raise ValueError("tape: expected actions of shape (steps, %d), got %s" % (self.batch_size, tuple(t.shape)))
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise AssertionError("actions must be integers")
        if t.dtype != torch.uint8:
            t = torch.where((t < 0) | (t > 255), torch.full_like(t, 255), t).to(torch.uint8)
        if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            t = t.contiguous()
        return t

    def collect_tape(self, actions, out=None, layout=None, stats=None):
        """`steps = len(actions)` consecutive step() calls with the CALLER's actions (pomdp_collect_tape*): row s of `actions`
        ([steps, N]; see as_tape) is what step() is handed at call counter t + s.  The fused launches of collect_synthetic /
        collect_returns — a lane's state in registers between its steps, up to 256 steps per launch — on actions the caller
        chose: a replayed trajectory, a table policy, another model's output.  Same results as a python loop over step(),
        row for row, including the final state.  layout "columns" (default): {"ob", "reward", "done"} [steps, N] (no action
        column: the caller holds it); "blocked" / "packed" / "narrow": as collect_synthetic; "returns" (or `stats` given): the
        episode statistics of collect_returns, returned as the EpisodeStats.  An action outside the env's range leaves the
        lane untouched for that step and is counted (invalid_action_count()).  auto_reset envs only.  Asynchronous."""
        if not self._has_reset:
            raise AttributeError("%s: collect before reset()" % type(self).__name__)
        if not self.auto_reset:
            raise ValueError("collect_tape needs auto_reset=True")
        self._check_driver_use("collect_tape")
        tape = self.as_tape(actions)
        steps, n = tape.shape[0], self.batch_size
        if stats is not None and layout is None:
            layout = "returns"
        if layout is None:
            layout = "columns" if out is None else out.get("layout", "columns")
        ct = _native.Tape(actions=tape.data_ptr(), stride=tape.stride(0) if steps > 1 else max(tape.stride(0), n))
        kind, t0 = _native.ENV_KIND[self.env_name], self._t
        self._t = t0 + steps
        with torch.cuda.device(self.device):
            if layout == "returns":
                if stats is None:
                    from ..history import EpisodeStats
                    stats = EpisodeStats(self)
                elif stats._n != n or stats.acc.device != self.device:
                    raise ValueError("collect_tape: `stats` belongs to another batch")
                rc = self._lib.pomdp_collect_tape_returns(kind, self._params_ref, self._ptrs[0], C.byref(ct), stats._ref, self._ptrs[4], n,
                                                          self._seed, self.lane_offset, t0, steps, _native.POMDP_AUTO_RESET, self._stream())
                _native.check(rc, "pomdp_collect_tape_returns")
                return stats
            if out is None:
                out = self.trajectory_buffers(steps, layout)
            if out.get("layout", "columns") != layout:
                raise ValueError("collect_tape: `out` was built for layout %r, not %r" % (out.get("layout", "columns"), layout))
            if layout == "columns":
                if not (out["ob"].shape[0] >= steps and out["ob"].shape[1] == n and out["reward"].shape == out["ob"].shape
                        and out["done_u8"].shape == out["ob"].shape):
                    raise ValueError("collect_tape: `out` does not have the shapes of trajectory_buffers(%d)" % steps)
                rc = self._lib.pomdp_collect_tape(kind, self._params_ref, self._ptrs[0], C.byref(ct), out["ob"].data_ptr(),
                                                  out["reward"].data_ptr(), out["done_u8"].data_ptr(), self._ptrs[4], n, self._seed,
                                                  self.lane_offset, t0, steps, n, _native.POMDP_AUTO_RESET, self._stream())
                _native.check(rc, "pomdp_collect_tape")
                return out
            traj, pitch = out["traj"], int(out["pitch"])
            row = {"blocked": (pitch * 13,), "packed": (pitch,), "narrow": (4, pitch)}[layout]
            if not (traj.shape[0] >= steps and tuple(traj.shape[1:]) == row and traj.is_contiguous() and pitch >= n):
                raise ValueError("collect_tape: `out` does not have the shape of trajectory_buffers(%d, %r)" % (steps, layout))
            rc = self._lib.pomdp_collect_tape_layout(kind, self._params_ref, self._ptrs[0], C.byref(ct), traj.data_ptr(), self._ptrs[4], n,
                                                     self._seed, self.lane_offset, t0, steps, pitch, _native.LAYOUTS[layout],
                                                     _native.POMDP_AUTO_RESET, self._stream())
            _native.check(rc, "pomdp_collect_tape_layout")
        return out

    def finish_episodes(self, steps, actions=None, layout="returns", out=None, stats=None):
        """Play the batch's episodes on: `steps` consecutive step() calls of an auto_reset=False env in one fused loop
        (pomdp_finish_episodes) — the synthetic uniform policy, or the CALLER's actions (`actions`: [steps, N], as_tape rules;
        steps = len(actions)).  A lane whose episode has ended (env.done) is frozen: it does not step, and every row of it
        reports (ob, reward, done) = (0, 0, 1), as step() does; env.done is updated in place.
        layout "returns" (default, or `stats` given): the episode statistics of collect_returns booked for live steps only —
        from a fresh EpisodeStats after reset(), stats.ret_done[i] is lane i's discounted return and stats.steps[i] its length;
        returns the EpisodeStats.  "packed" / "narrow": the trajectory (trajectory_buffers; decode_trajectory works), frozen
        rows padded; returns the dict.  `out` / `stats` continue an earlier call.  Then reset(where=env.done) restarts the
        finished lanes.  auto_reset=False envs only.  Asynchronous: there is no early stop on the host."""
        if not self._has_reset:
            raise AttributeError("%s: finish_episodes before reset()" % type(self).__name__)
        if self.auto_reset:
            raise ValueError("finish_episodes needs auto_reset=False (an auto-reset env never finishes)")
        self._check_driver_use("finish_episodes")
        n = self.batch_size
        if n == 1:
            raise ValueError("finish_episodes: a batch of one keeps its done flag on the host — use step()")
        if stats is not None:
            layout = "returns"
        elif out is not None:
            layout = out.get("layout", "columns")
        if layout not in ("returns", "packed", "narrow"):
            raise ValueError("finish_episodes: layout must be 'returns', 'packed' or 'narrow', got %r" % (layout,))
        tape = ct = None
        if actions is not None:
            tape = self.as_tape(actions)
            steps = tape.shape[0]
            ct = _native.Tape(actions=tape.data_ptr(), stride=tape.stride(0) if steps > 1 else max(tape.stride(0), n))
        steps = int(steps)
        args = _native.EpisodeArgs(env=_native.ENV_KIND[self.env_name], layout=0, params=C.addressof(self._params),
                                   state=self._ptrs[0], done=self._ptrs[3], tape=C.addressof(ct) if ct is not None else None,
                                   traj=None, pitch=0, stats=None, err=self._ptrs[4], n=n, seed=self._seed,
                                   lane0=self.lane_offset, reserved=0)
        with torch.cuda.device(self.device):
            if layout == "returns":
                if stats is None:
                    from ..history import EpisodeStats
                    stats = EpisodeStats(self)
                elif stats._n != n or stats.acc.device != self.device:
                    raise ValueError("finish_episodes: `stats` belongs to another batch")
                args.layout, args.stats = _native.POMDP_LAYOUT_RETURNS, C.addressof(stats._ptrs)
                result = stats
            else:
                if out is None:
                    out = self.trajectory_buffers(steps, layout)
                traj, pitch = out["traj"], int(out["pitch"])
                row = {"packed": (pitch,), "narrow": (4, pitch)}[layout]
                if not (traj.shape[0] >= steps and tuple(traj.shape[1:]) == row and traj.is_contiguous() and pitch >= n
                        and traj.dtype == (torch.int32 if layout == "packed" else torch.uint8)):
                    raise ValueError("finish_episodes: `out` does not have the shape of trajectory_buffers(%d, %r)" % (steps, layout))
                args.layout, args.traj, args.pitch = _native.LAYOUTS[layout], traj.data_ptr(), pitch
                result = out
            t0 = self._t
            self._t = t0 + steps
            rc = self._lib.pomdp_finish_episodes(C.byref(args), t0, steps, self._stream())
            _native.check(rc, "pomdp_finish_episodes")
        self.done = self._done_bool
        return result

    def run_controller(self, ctrl, steps, layout="returns", out=None, stats=None):
        """finish_episodes under a policy that reacts to what each lane observes: `steps` consecutive step() calls of an
        auto_reset=False env in one fused loop (pomdp_controller_episodes), lane i taking ctrl.action[ctrl.node[i]] and then
        moving to ctrl.next[ctrl.node[i]][ob] (`ctrl`: a gym_pomdp_amd.Controller of this env; ctrl.node is updated in place,
        so a later call goes on where this one stopped) — or, under a gym_pomdp_amd.StochasticController, drawing both among
        the node's candidates (pomdp_stoch_controller_episodes).  Same draws as step() at the same call counters, same frozen rows,
        layouts, `out` / `stats` and return values as finish_episodes; env.done is updated in place.  An entry a
        validate=False controller should not hold — an action out of range, a successor that is no node — is handled as
        include/pomdp_hip.h says and counted in invalid_action_count().  Then ctrl.reset_nodes(where=env.done) followed by
        reset(where=env.done) restarts the finished lanes (in that order: the reset clears env.done).  auto_reset=False envs
        only.  Asynchronous."""
        if not self._has_reset:
            raise AttributeError("%s: run_controller before reset()" % type(self).__name__)
        if self.auto_reset:
            raise ValueError("run_controller needs auto_reset=False (an auto-reset env never finishes)")
        self._check_driver_use("run_controller")
        n = self.batch_size
        if n == 1:
            raise ValueError("run_controller: a batch of one keeps its done flag on the host — use step()")
        if getattr(ctrl, "env", None) is not self:
            raise ValueError("run_controller: `ctrl` was built for another env")
        if stats is not None:
            layout = "returns"
        elif out is not None:
            layout = out.get("layout", "columns")
        if layout not in ("returns", "packed", "narrow"):
            raise ValueError("run_controller: layout must be 'returns', 'packed' or 'narrow', got %r" % (layout,))
        steps = int(steps)
        args = _native.EpisodeArgs(env=_native.ENV_KIND[self.env_name], layout=0, params=C.addressof(self._params),
                                   state=self._ptrs[0], done=self._ptrs[3], tape=None, traj=None, pitch=0, stats=None,
                                   err=self._ptrs[4], n=n, seed=self._seed, lane0=self.lane_offset, reserved=0)
        entry, cargs = ctrl._native_call()                   # Controller: pomdp_controller_episodes; StochasticController: its own
        with torch.cuda.device(self.device):
            if layout == "returns":
                if stats is None:
                    from ..history import EpisodeStats
                    stats = EpisodeStats(self)
                elif stats._n != n or stats.acc.device != self.device:
                    raise ValueError("run_controller: `stats` belongs to another batch")
                args.layout, args.stats = _native.POMDP_LAYOUT_RETURNS, C.addressof(stats._ptrs)
                result = stats
            else:
                if out is None:
                    out = self.trajectory_buffers(steps, layout)
                traj, pitch = out["traj"], int(out["pitch"])
                row = {"packed": (pitch,), "narrow": (4, pitch)}[layout]
                if not (traj.shape[0] >= steps and tuple(traj.shape[1:]) == row and traj.is_contiguous() and pitch >= n
                        and traj.dtype == (torch.int32 if layout == "packed" else torch.uint8)):
                    raise ValueError("run_controller: `out` does not have the shape of trajectory_buffers(%d, %r)" % (steps, layout))
                args.layout, args.traj, args.pitch = _native.LAYOUTS[layout], traj.data_ptr(), pitch
                result = out
            t0 = self._t
            self._t = t0 + steps
            rc = getattr(self._lib, entry)(C.byref(args), C.byref(cargs), t0, steps, self._stream())
            _native.check(rc, entry)
        self.done = self._done_bool
        return result

    def _check_driver_use(self, what):
        """The C-side episode loops advance the packed state only: they know nothing of RockSample's side statistics
        (use_heuristic / track_belief envs), and the synthetic policy shares one Philox block among global lanes
        4q .. 4q+3, so a shard has to start on such a boundary."""
        if self._tracker is not None:
            raise ValueError("%s: this env maintains RockSample's side statistics (use_heuristic / track_belief), which "
                             "the C-side drivers do not update — use step() or heuristic_steps()" % what)
        if self.lane_offset % 4:
            raise ValueError("%s: lane_offset must be a multiple of 4 (got %d): the synthetic policy's Philox block is "
                             "shared by global lanes 4q .. 4q+3" % (what, self.lane_offset))

    def collect_synthetic(self, steps, out=None, layout=None):
        """`steps` consecutive step() calls under the synthetic uniform policy with every step's results KEPT
        (pomdp_collect_synthetic): returns {"action": int32 [steps + 1, N] (row s = the actions of step s, last row = the
        next call's), "ob": int32 [steps, N], "reward": [steps, N], "done": bool [steps, N]} — row s equals what
        synthetic_actions() + step() return at that call.  The batched form of the reference callers' episode
        loops (rock.py:553-575); up to pomdp_fuse_steps(env, layout) steps per launch (256; 64 for the 13-byte layouts of RockSample /
        Tag / Tiger), auto_reset envs only.  `out`: a dict from an earlier call
        to write into.  `layout` (default: `out`'s, else "columns"): "blocked" / "packed" / "narrow" write the same
        information as one stream per step (pomdp_collect_layout; trajectory_buffers, decode_trajectory).  Asynchronous."""
        if not self._has_reset:
            raise AttributeError("%s: collect before reset()" % type(self).__name__)
        if not self.auto_reset:
            raise ValueError("collect_synthetic needs auto_reset=True")
        self._check_driver_use("collect_synthetic")
        steps, n = int(steps), self.batch_size
        if layout is None:
            layout = "columns" if out is None else out.get("layout", "columns")
        if out is None:
            out = self.trajectory_buffers(steps, layout)
        if out.get("layout", "columns") != layout:
            raise ValueError("collect_synthetic: `out` was built for layout %r, not %r" % (out.get("layout", "columns"), layout))
        if layout != "columns":
            return self._collect_traj(steps, out, layout)
        if not (out["action"].shape == (steps + 1, n) and out["ob"].shape == (steps, n) and out["reward"].shape == (steps, n)
                and out["done_u8"].shape == (steps, n)):
            raise ValueError("collect_synthetic: `out` does not have the shapes of trajectory_buffers(%d)" % steps)
        # the call's per-buffer arguments (include/pomdp_hip.h: pomdp_collect_args), bound once per set of buffers: the
        # cache lives on the env and is keyed by the buffers' addresses, so a dict handed to another env, or one whose
        # tensors were replaced, never meets a stale struct
        key = (out["action"].data_ptr(), out["ob"].data_ptr(), out["reward"].data_ptr(), out["done_u8"].data_ptr(), steps)
        bound = self._collect_cache.get(key)
        if bound is None:
            if len(self._collect_cache) >= 64:
                self._collect_cache.clear()
            a = _native.CollectArgs(env=_native.ENV_KIND[self.env_name], flags=_native.POMDP_AUTO_RESET,
                                    params=C.addressof(self._params), state=self._ptrs[0], action=key[0],
                                    ob=key[1], reward=key[2], done=key[3],
                                    err=self._ptrs[4], n=n, pitch=n, seed=self._seed,
                                    lane0=self.lane_offset, reserved=0)
            bound = self._collect_cache[key] = (a, C.byref(a), steps)
        bound[0].seed = self._seed
        t0 = self._t
        self._t = t0 + steps
        if _current_device() == self._dev_index:         # no device-context switch on the common path
            rc = self._lib.pomdp_collect(bound[1], t0, steps, _raw_stream(self._dev_index))
        else:
            with torch.cuda.device(self.device):
                rc = self._lib.pomdp_collect(bound[1], t0, steps, self._stream())
        if rc:
            _native.check(rc, "pomdp_collect_synthetic")
        return out

    def _collect_traj(self, steps, out, layout):
        """collect_synthetic into a blocked / packed / narrow trajectory: pomdp_collect_traj with its arguments bound per buffer."""
        n, traj, pitch = self.batch_size, out["traj"], int(out["pitch"])
        row = {"blocked": (pitch * 13,), "packed": (pitch,), "narrow": (4, pitch)}[layout]
        if not (traj.shape[0] >= steps and tuple(traj.shape[1:]) == row and traj.is_contiguous() and pitch >= n
                and traj.dtype == (torch.int32 if layout == "packed" else torch.uint8)):
            raise ValueError("collect_synthetic: `out` does not have the shape of trajectory_buffers(%d, %r)" % (steps, layout))
        key = (traj.data_ptr(), layout, pitch)
        bound = self._collect_cache.get(key)
        if bound is None:
            if len(self._collect_cache) >= 64:
                self._collect_cache.clear()
            a = _native.TrajArgs(env=_native.ENV_KIND[self.env_name], flags=_native.POMDP_AUTO_RESET, layout=_native.LAYOUTS[layout],
                                 reserved=0, params=C.addressof(self._params), state=self._ptrs[0], traj=key[0], err=self._ptrs[4],
                                 n=n, pitch=pitch, seed=self._seed, lane0=self.lane_offset, reserved2=0)
            bound = self._collect_cache[key] = (a, C.byref(a), steps)
        bound[0].seed = self._seed
        t0 = self._t
        self._t = t0 + steps
        if _current_device() == self._dev_index:
            rc = self._lib.pomdp_collect_traj(bound[1], t0, steps, _raw_stream(self._dev_index))
        else:
            with torch.cuda.device(self.device):
                rc = self._lib.pomdp_collect_traj(bound[1], t0, steps, self._stream())
        if rc:
            _native.check(rc, "pomdp_collect_layout")
        return out

    def __repr__(self):
        return "%s(batch_size=%d, device=%s)" % (type(self).__name__, self.batch_size, getattr(self, "device", "?"))
