"""GPU parity of the kernels bench.py TIMES — the fused multi-step launches behind env.collect_synthetic /
env.rollout_synthetic(fuse=True) (steps_quad_kernel, tag_steps_quad_kernel, steps_quad_generic_kernel, steps_kernel) and
the fused rollout kernel — against the CPU oracle DIRECTLY: every row of every collected step over the whole batch, at
BASELINE.json's per-GPU sizes (metric: RockSample(7,8) 2^20 lanes; C3 Tag 2^20; C4 BattleShip 10x10 2^19 lanes per GPU;
C5 RockSample(15,15) 2^21 simulations per GPU = 2048 roots x 1024).  Plus: env.seed(), and the bench command the driver
runs (single GPU with --steps 20 --warmup 5, and --gpus 2 self-launched with both ranks on the one visible GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import history_window_restatement as hw
from conftest import REPO
from test_gpu_parity import make_env, np_

pytestmark = pytest.mark.gpu

FULL = [("rock", {}, 1 << 20, 70), ("rock", dict(board_size=15, num_rocks=15), 1 << 20, 70), ("tag", {}, 1 << 20, 70),
        ("tiger", {}, 1 << 20, 70), ("network", {}, 1 << 20, 70),
        ("battleship", dict(board_size=(10, 10), max_len=5), 1 << 19, 70),            # C4: 2^22 lanes over 8 GPUs
        ("stochrock", {}, 1 << 18, 70), ("stochrock", {}, 1 << 19, 70), ("stochrock", dict(board_size=15, num_rocks=15), 1 << 19, 40),
        ("battleship", {}, 1 << 18, 70), ("battleship", {}, 1 << 16, 70), ("battleship", dict(board_size=(10, 10), max_len=5), 1 << 16, 70),   # the quad loop's gate (2^16)
        # the shards a 2^20-lane batch leaves per GPU at 2, 4 and 8 GPUs
        ("rock", {}, 1 << 19, 66), ("rock", {}, 1 << 18, 66), ("rock", {}, 1 << 17, 66),
        ("rock", {}, 3 << 18, 66), ("rock", dict(board_size=15, num_rocks=15), 1 << 19, 66),   # either side of RockSample's quad gate (3 * 2^18 lanes)
        ("tag", {}, 1 << 17, 66), ("tag", {}, 1 << 19, 66), ("tiger", {}, 1 << 17, 66), ("tiger", {}, 1 << 18, 66), ("tiger", {}, 1 << 19, 66),
        ("network", {}, 1 << 17, 66), ("network", {}, 1 << 18, 66), ("network", {}, 1 << 19, 66),
        # Network's quad-per-thread loop with streams that run past their first block on most lanes
        ("network", dict(n_machines=16, problem_type=1), 1 << 19, 40), ("network", dict(n_machines=31, problem_type=3), 1 << 19, 40),
        # BattleShip on boards whose episodes are short (resets in most waves at every step)
        ("battleship", {}, 1 << 19, 130), ("battleship", dict(board_size=(8, 6), max_len=4), 1 << 19, 70),
        ("battleship", dict(board_size=(10, 10), max_len=5), 1 << 20, 20),
        # batches that are not a multiple of 4 (the last shard of an odd total): ragged last workgroup, scalar tail of the first actions
        ("rock", {}, 4099, 70), ("tag", {}, (1 << 18) + 5, 20), ("network", {}, 777, 70), ("tiger", {}, 3, 70),
        ("battleship", {}, 259, 70),
        # the non-default configs inside the fused kernels (until round 3 they met the oracle only through HIP-vs-HIP tests):
        # several opponents in steps_kernel<TagEnv, 2, true> (tag.py:119-130 loops over them), the other table sizes of
        # steps_quad_kernel (rock.py:43-64: an odd K, a table of 8 actions), and the driver's exact 20-step launch
        ("tag", dict(num_opponents=2), 1 << 20, 40), ("tag", dict(num_opponents=4), 1 << 20, 40),
        ("rock", dict(board_size=11, num_rocks=11), 1 << 20, 66), ("rock", dict(board_size=7, num_rocks=7), 1 << 20, 66),
        ("rock", dict(board_size=4, num_rocks=3), 1 << 20, 66), ("rock", {}, 1 << 20, 20)]


@pytest.fixture
def fuse64():
    """64 steps per fused launch (the default is 256: include/pomdp_hip.h, pomdp_fuse_max), so that a 66-130 step collection
    crosses launch boundaries — results never depend on the launch length, which is what these tests then also check."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    L.pomdp_fuse_max(64)
    yield
    L.pomdp_fuse_max(_native.FUSE_MAX_DEFAULT)


@pytest.mark.parametrize("env,kw,n,steps", FULL, ids=["%s%s-%d" % (c[0], "-".join(str(v) for v in c[1].values()), c[2]) for c in FULL])
def test_collected_rows_equal_the_oracle(oracle_lib, fuse64, env, kw, n, steps):
    """collect_synthetic(steps) — what bench.py's timed region calls — against oracle.batch_step fed with the synthetic
    policy's actions: every row (action, ob, reward, done) over the whole batch, across the 64-step launch boundary, then
    the final state."""
    seed, lane0, t0 = 20260929, 1 << 22, (1 << 33) + 5
    nt = oracle_lib.max_threads()
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
    e.call_counter = t0
    o = oracle_lib.OracleEnv(env, **kw)
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, t0, nthreads=nt))
    tr = e.collect_synthetic(steps)
    done = np.zeros(n, np.uint8)
    for k in range(steps):
        t = t0 + 1 + k
        a = oracle_lib.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt)
        ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
        ctx = (env, kw, n, k)
        assert bad == 0, ctx
        assert np.array_equal(np_(tr["action"][k]), a), ctx
        assert np.array_equal(np_(tr["ob"][k]), ob), ctx
        assert np.array_equal(np_(tr["reward"][k]), rew), ctx
        assert np.array_equal(np_(tr["done"][k]), done.astype(bool)), ctx
    assert np.array_equal(np_(tr["action"][steps]), oracle_lib.synthetic_actions(n, seed, lane0, t0 + 1 + steps, o.n_actions, nthreads=nt))
    assert np.array_equal(np_(e.state).view(np.uint32), st)
    assert e.invalid_action_count() == 0


# ---- fused launches over the CALLER's actions (pomdp_collect_tape*) ---------------------------------------------------------
TAPES = [("rock", {}, 1 << 20, 80), ("rock", dict(board_size=15, num_rocks=15), 1 << 20, 40), ("stochrock", {}, 1 << 19, 40),
         ("tag", {}, 1 << 20, 70), ("tiger", {}, 1 << 20, 70), ("network", {}, 1 << 20, 40),
         ("battleship", dict(board_size=(10, 10), max_len=5), 1 << 19, 70), ("battleship", {}, 1 << 18, 70),
         # below the quad gates / ragged / several opponents: the general one-lane-per-thread loop
         ("rock", {}, 1 << 17, 66), ("rock", {}, 4099, 70), ("tag", dict(num_opponents=2), 1 << 18, 40), ("tiger", {}, 3, 70),
         ("network", dict(n_machines=16, problem_type=1), 777, 40), ("battleship", {}, 259, 70),
         # RockSample's half-quad-per-thread loop (7 * 2^16 .. 3 * 2^18 lanes)
         ("rock", {}, 1 << 19, 80), ("rock", dict(board_size=15, num_rocks=15), 5 << 17, 40),
         # ... and Tag's (3 * 2^17 .. 3 * 2^18 - 1 lanes)
         ("tag", {}, 1 << 19, 80), ("tag", {}, 3 << 17, 40),
         # full workgroups below the quad gates: the small shards' loops with the tape read four rows ahead (RockSample's table-driven
         # step from 16 steps per launch: 66 = 64 + 2, the last launch takes the table-free form)
         ("rock", dict(board_size=15, num_rocks=15), 1 << 18, 66), ("rock", {}, 5120, 37), ("tiger", {}, 1 << 17, 70),
         ("tag", {}, 1 << 17, 66), ("network", {}, 1 << 18, 40), ("network", dict(n_machines=16, problem_type=1), 2048, 23)]


def _tape(rng, n_actions, steps, n, bad_every):
    """a tape no policy of ours produced: uniform actions from numpy, with an out-of-range byte (n_actions .. 255) on one lane-step in `bad_every`"""
    tape = rng.randint(0, n_actions, (steps, n)).astype(np.uint8)
    if bad_every:
        bad = rng.randint(0, bad_every, (steps, n)) == 0
        tape[bad] = rng.randint(n_actions, 256, int(bad.sum())).astype(np.uint8)
    return tape


@pytest.mark.parametrize("env,kw,n,steps", TAPES, ids=["%s%s-%d" % (c[0], "-".join(str(v) for v in c[1].values()), c[2]) for c in TAPES])
@pytest.mark.parametrize("layout", ["packed", "columns"])
def test_tape_driven_rows_equal_the_oracle(oracle_lib, fuse64, env, kw, n, steps, layout):
    """collect_tape(actions): the fused launches on the CALLER's actions (rock.py:562-566: `env.step(action)` with whatever the
    caller chose) against oracle.batch_step fed the same tape — every row over the whole batch, across the 64-step launch
    boundary, out-of-range bytes included (lane untouched, (0, 0, 0), counted), then the final state."""
    seed, lane0, t0 = 77001, 1 << 21, (1 << 32) - 9
    nt = oracle_lib.max_threads()
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
    e.call_counter = t0
    o = oracle_lib.OracleEnv(env, **kw)
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, t0, nthreads=nt))
    tape = _tape(np.random.RandomState(n % 9973 + steps), o.n_actions, steps, n, 4096)
    tr = e.collect_tape(torch.as_tensor(tape, device="cuda"), layout=layout)
    cols = e.decode_trajectory(tr, steps)
    done, n_bad = np.zeros(n, np.uint8), 0
    for k in range(steps):
        a = tape[k].astype(np.int32)
        ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t0 + 1 + k, auto_reset=True, done=done, nthreads=nt)
        n_bad += bad
        ctx = (env, kw, n, k, layout)
        if layout == "packed":
            assert np.array_equal(np_(cols["action"][k]), a), ctx          # the record keeps the byte it was given
        assert np.array_equal(np_(cols["ob"][k]), ob), ctx
        assert np.array_equal(np_(cols["reward"][k]), rew), ctx
        assert np.array_equal(np_(cols["done"][k]), done.astype(bool)), ctx
    assert np.array_equal(np_(e.state).view(np.uint32), st)
    assert e.invalid_action_count() == n_bad == int((tape >= o.n_actions).sum())
    want_kernel = {"rock": "steps_quad_kernel", "stochrock": "steps_quad_kernel", "tag": "tag_steps_quad_kernel", "tiger": "steps_quad_generic_kernel",
                   "network": "network_steps_quad_kernel", "battleship": "battleship_steps_quad_kernel"}[env]
    from gym_pomdp_amd import _native
    name = _native.lib().pomdp_last_fused_kernel().decode()
    assert name.endswith(", Tape>") or ", Tape" in name, name
    # the quad-per-thread loops' gates (kernels_common.hip.h); RockSample's records ride the half-quad form from above 3 * 2^17 lanes
    quad_from = {"battleship": 1 << 16, "rock": (3 << 17) + 1 if layout == "packed" else 3 << 18,
                 "tag": 3 << 17 if layout == "packed" and kw.get("num_opponents", 1) == 1 else 1 << 19}.get(env, 1 << 19)
    if n >= quad_from:
        assert name.startswith(want_kernel + "<"), name                    # the quad-per-thread loop took it
    elif n < 1 << 16 or n % 1024:
        assert name.startswith("steps_kernel<"), name


@pytest.mark.parametrize("env,kw,n", [("rock", {}, 1 << 20), ("tag", {}, 1 << 19), ("network", {}, 1 << 19), ("tiger", {}, 1000),
                                      ("battleship", dict(board_size=(10, 10), max_len=5), 1 << 17)], ids=["rock", "tag", "network", "tiger-ragged", "battleship"])
def test_tape_driven_returns_and_other_sinks(oracle_lib, fuse64, env, kw, n):
    """The returns sink on a tape (float64 statistics bit for bit against or_batch_collect_returns fed the same tape, out-of-range
    bytes booking a step with reward 0) and the narrow / blocked sinks (== the packed rows); then a replay: the action plane
    of a narrow trajectory collected under the synthetic policy, fed back as a tape with its 4 * pitch row stride, reproduces
    that trajectory and its final state."""
    seed, lane0, steps = 4711, 8192, 150
    nt = oracle_lib.max_threads()
    o = oracle_lib.OracleEnv(env, **kw)
    tape = _tape(np.random.RandomState(5), o.n_actions, steps, n, 1000)
    d_tape = torch.as_tensor(tape, device="cuda")
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, 0, nthreads=nt))
    stats = e.collect_tape(d_tape, layout="returns")
    acc, cnt = oracle_lib.new_return_stats(n, stats.acc.shape[1])
    o.batch_collect_returns(st, acc, cnt, e._discount, seed, lane0, 1, steps, nthreads=nt, actions=tape.astype(np.int32))
    assert np.array_equal(np_(stats.acc)[:, :n].view(np.uint64), acc[:, :n].view(np.uint64))
    assert np.array_equal(np_(stats.cnt)[:, :n], cnt[:, :n]) and np.array_equal(np_(e.state).view(np.uint32), st)
    want = None
    for layout in ("packed", "narrow", "blocked"):
        f = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
        f.reset()
        cols = f.decode_trajectory(f.collect_tape(d_tape, layout=layout), steps)
        got = {k: np_(v).astype(np.float64) for k, v in cols.items()}
        if want is None:
            want = got
        for k in want:
            assert np.array_equal(got[k], want[k]), (layout, k)
        assert np.array_equal(np_(f.state).view(np.uint32), st)
    # replay
    a = make_env(env, kw, batch_size=n, seed=seed + 1, lane_offset=lane0, reuse_buffers=True)
    b = make_env(env, kw, batch_size=n, seed=seed + 1, lane_offset=lane0, reuse_buffers=True)
    a.reset(), b.reset()
    tr = a.collect_synthetic(steps, layout="narrow")
    plane = tr["traj"][:, 0, :n]                                          # uint8 [steps, n], row stride 4 * pitch: used in place
    assert b.as_tape(plane).data_ptr() == plane.data_ptr()
    rp = b.collect_tape(plane, layout="narrow")
    assert torch.equal(rp["traj"][:, :, :n], tr["traj"][:, :, :n]) and torch.equal(a.state, b.state) and b.invalid_action_count() == 0


def test_tape_through_the_c_abi_and_host_checks():
    """pomdp_collect_tape* called directly: argument checks, an unaligned tape (the general loop), and the host-side conversions."""
    import ctypes as C
    from gym_pomdp_amd import _native
    L = _native.lib()
    n, k = 2048, 20
    e = make_env("rock", {}, batch_size=n, seed=3, reuse_buffers=True)
    e.reset()
    ref = make_env("rock", {}, batch_size=n, seed=3, reuse_buffers=True)
    ref.reset()
    raw = torch.randint(0, 13, (k, n + 3), dtype=torch.uint8, device="cuda")
    tape = raw[:, 3:]                                                     # rows start 3 bytes off a 4-byte boundary, stride n + 3
    bufs = e.trajectory_buffers(k)
    ct = _native.Tape(actions=tape.data_ptr(), stride=n + 3)
    args = (_native.ENV_KIND["rock"], e._params_ref, e.state.data_ptr())
    tail = (bufs["ob"].data_ptr(), bufs["reward"].data_ptr(), bufs["done_u8"].data_ptr(), e._err.data_ptr(), n, 3, 0, 1, k, n)
    assert L.pomdp_collect_tape(*args, None, *tail, 1, None) == -1
    assert L.pomdp_collect_tape(*args, C.byref(ct), *tail, 0, None) == -1                 # auto-reset is required
    assert L.pomdp_collect_tape(*args, C.byref(_native.Tape(actions=tape.data_ptr(), stride=n - 1)), *tail, 1, None) == -1
    assert L.pomdp_collect_tape(*args, C.byref(_native.Tape(actions=None, stride=n)), *tail, 1, None) == -1
    assert L.pomdp_collect_tape(*args, C.byref(ct), *tail, 1, None) == 0
    assert _native.lib().pomdp_last_fused_kernel().decode().startswith("steps_kernel<")
    for s in range(k):
        ob, rew, done, _ = ref.step(tape[s].to(torch.int32))
        assert torch.equal(bufs["ob"][s], ob) and torch.equal(bufs["reward"][s], rew) and torch.equal(bufs["done"][s], done), s
    assert torch.equal(e.state, ref.state)
    # host side: wide integers, lists, numpy; floats are refused like step() refuses them
    t = e.as_tape(torch.tensor([[0, 300, -1, 12] + [1] * (n - 4)], dtype=torch.int64))
    assert t.dtype == torch.uint8 and t[0, :4].tolist() == [0, 255, 255, 12]
    assert e.as_tape(np.zeros((2, n), np.int32)).shape == (2, n)
    with pytest.raises(AssertionError):
        e.as_tape(torch.zeros((2, n)))
    with pytest.raises(ValueError):
        e.as_tape(torch.zeros((2, n - 1), dtype=torch.uint8))
    frozen = make_env("rock", {}, batch_size=n, seed=3, auto_reset=False)
    with pytest.raises(AttributeError):
        frozen.collect_tape(tape)                                          # before reset(), like step()
    frozen.reset()
    with pytest.raises(ValueError):
        frozen.collect_tape(tape)                                          # auto_reset envs only


@pytest.mark.parametrize("env,kw,n", [("rock", {}, 1 << 20), ("tag", {}, 1 << 20), ("network", {}, 1 << 18), ("network", {}, 1 << 19),
                                      ("battleship", {}, 1 << 19)],
                         ids=["rock", "tag", "network", "network-quad", "battleship"])
def test_fused_overwrite_mode_equals_the_oracle(oracle_lib, fuse64, env, kw, n):
    """rollout_synthetic(fuse=True) (bench.py --collect 0): after k fused steps the N-element outputs hold the LAST step's
    results and `actions` the following call counter's — against the oracle."""
    seed, lane0 = 31337, 4096
    nt = oracle_lib.max_threads()
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
    o = oracle_lib.OracleEnv(env, **kw)
    st = o.new_state(n)
    o.batch_reset(st, seed, lane0, 0, nthreads=nt)
    e.reset()
    done, t = np.zeros(n, np.uint8), 1
    for k in (20, 64, 3):
        ob_g, rew_g, done_g = e.rollout_synthetic(k, fuse=True)
        for _ in range(k):
            a = oracle_lib.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt)
            ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
            t += 1
        assert np.array_equal(np_(ob_g), ob) and np.array_equal(np_(rew_g), rew) and np.array_equal(np_(done_g), done.astype(bool)), (env, k)
        assert np.array_equal(np_(e._action_scratch), oracle_lib.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt))
        assert np.array_equal(np_(e.state).view(np.uint32), st), (env, k)


def test_network_ties_inside_the_fused_launch(oracle_lib):
    """Lanes whose first step has a draw decided by its low word (tests/golden/ties_network.npz, found by find_ties.py; the
    oracle's handling of them is pinned to the reference there) inside a batch large enough for network_steps_quad_kernel:
    draw 2 lies in the block every lane computes (-> the exact per-lane form), draws 4, 5 and 9 in the pooled continuation."""
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "ties_network.npz")))
    seed, n = int(g["seed"]), 1 << 19
    o = oracle_lib.OracleEnv("network")
    for lane, draw in zip(g["lanes"], g["tied_draw"]):
        lane = int(lane)
        lane0 = max(0, (lane & ~1023) - 4096)
        e = make_env("network", {}, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
        e.reset()
        tr = e.collect_synthetic(16)
        w0, wn = lane - 8 - (lane & 3), 32                                  # a window of whole quads around the lane
        st = o.new_state(wn)
        o.batch_reset(st, seed, w0, 0)
        for k in range(16):
            a = oracle_lib.synthetic_actions(wn, seed, w0, 1 + k, o.n_actions)
            ob, rew, done, bad = o.batch_step(st, a, seed, w0, 1 + k)
            sl = slice(w0 - lane0, w0 - lane0 + wn)
            assert np.array_equal(np_(tr["action"][k, sl]), a), (lane, draw, k)
            assert np.array_equal(np_(tr["ob"][k, sl]), ob) and np.array_equal(np_(tr["reward"][k, sl]), rew), (lane, draw, k)
        assert np.array_equal(np_(e.state[:, sl]).view(np.uint32), st), (lane, draw)


def test_rollouts_at_the_c5_per_gpu_size(oracle_lib):
    """BASELINE.json configs[4] per GPU: RockSample(15,15), 2048 roots x 1024 simulations = 2^21 lanes, one fused rollout
    launch — every simulation's return (float64, bit for bit), length, first action, last observation and termination."""
    kw, roots, sims, depth = dict(board_size=15, num_rocks=15), 2048, 1024, 64
    seed, lane0 = 55, 1 << 21                                            # the second GPU's lane range
    nt = oracle_lib.max_threads()
    o = oracle_lib.OracleEnv("rock", **kw)
    e = make_env("rock", kw, batch_size=roots, seed=seed, lane_offset=lane0)
    st = o.new_state(roots)
    o.batch_reset(st, seed, lane0, 0, nthreads=nt)
    e.reset()
    for _ in range(4):
        a = oracle_lib.synthetic_actions(roots, seed, lane0, e.call_counter, o.n_actions)
        o.batch_step(st, a, seed, lane0, e.call_counter, nthreads=nt)
        e.step(torch.as_tensor(a, device="cuda"))
    assert np.array_equal(np_(e.state).view(np.uint32), st)
    t0 = e.call_counter
    want = o.batch_rollout(st, sims, depth, e._discount, seed, lane0, t0, nthreads=nt)
    got = e.rollout(depth, sims_per_root=sims)
    assert np.array_equal(np_(got["ret"]).view(np.uint64), want["ret"].view(np.uint64))
    for k in ("n_steps", "first_action", "last_ob"):
        assert np.array_equal(np_(got[k]), want[k]), k
    assert np.array_equal(np_(got["terminated"]), want["terminated"].astype(bool))
    assert int(want["n_steps"].sum()) > roots * sims                      # the simulations really ran


@pytest.mark.parametrize("env,kw", [("rock", {}), ("tag", {}), ("battleship", {}), ("tiger", {}), ("network", {})],
                         ids=["rock", "tag", "battleship", "tiger", "network"])
def test_seed_call_equals_a_fresh_env(env, kw):
    """a16: env.seed(s) (rock.py:120-121 etc.) puts an env that already ran where a fresh env built with seed=s starts:
    same reset observation, same trajectory; and returns [s] like gym's seed()."""
    n = 4096
    used = make_env(env, kw, batch_size=n, seed=1, lane_offset=64)
    used.reset()
    for _ in range(5):
        used.step(used.synthetic_actions())
    assert used.seed(987654321) == [987654321]
    fresh = make_env(env, kw, batch_size=n, seed=987654321, lane_offset=64)
    assert torch.equal(used.reset(), fresh.reset()) and torch.equal(used.state, fresh.state)
    for _ in range(12):
        a = fresh.synthetic_actions()
        assert torch.equal(used.synthetic_actions(), a)
        ra, rb = used.step(a), fresh.step(a)
        assert all(torch.equal(x, y) for x, y in zip(ra[:3], rb[:3]))
        assert torch.equal(used.state, fresh.state)
    one, two = make_env(env, kw, seed=3), make_env(env, kw, seed=99)     # scalar mode (the reference's usage)
    one.reset()
    one.step(0)
    one.seed(99)
    assert one.reset() == two.reset()
    assert one.step(1)[:3] == two.step(1)[:3]


def _bench(*argv, timeout=900):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + [str(a) for a in argv], capture_output=True, text=True,
                         timeout=timeout, cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_as_the_driver_runs_it():
    """`python bench.py --gpus 1 --steps 20 --warmup 5`: ONE JSON line with the contract's keys, and the figures of the
    timed region — no allocation inside it, the fused kernel named as a profiler shows it, the per-step time and roofline
    fraction of the committed profiles (within the spread of a short region); the other trajectory layouts and
    BASELINE.json's configs[2..4] measured in the same run."""
    d = _bench("--gpus", 1, "--steps", 20, "--warmup", 5, "--cpu-seconds", 2)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "layouts", "configs"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert d["config"]["seeds"] == [0, 1, 2] and d["config"]["repeats"] >= 30 and len(d["config"]["seed_values"]["per_seed"]) == 3
    assert d["config"]["trajectories_kept"] is True and d["config"]["trajectory_layout"] == "packed"
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "hbm", "valu"):
        assert k in r, k
    assert r["bound"] in ("hbm", "valu") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["frac"] <= 1.0
    assert r["kernel"].startswith("steps_quad_kernel<RockEnv<1>, Packed>"), r["kernel"]
    assert r["kernel_ms"] < 2.1e-3, r                                  # profiles: 1.86-1.88 us per step of a 20-step launch
    assert d["ms_per_step"] < 3.6e-3, d["ms_per_step"]                 # by wall clock, launch + sync wake-up included
    h = r["hbm"]
    assert h["bound"] == "hbm" and abs(h["frac"] - h["achieved"] / h["peak"]) < 1e-9 and abs(r["algorithmic_bytes_per_step"] - 4.4) < 1e-9
    v = r["valu"]
    if v is not None:       # the kernel's VALU count is on record: instructions per launch / this run's launch time, and its staleness
        assert v["bound"] == "valu" and v["unit"] == "wave-instructions/s" and abs(v["frac"] - v["achieved"] / v["peak"]) < 1e-9
        assert 0.65 < v["frac"] <= 1.0 and r["tighter_bound"] in ("valu", "hbm") and isinstance(r["counters_stale"], bool), v
        if not r["counters_stale"]:
            assert r["bound"] == r["tighter_bound"]
            # the recorded HBM bytes of THIS launch shape (20 steps, packed records)
            assert r["traffic"] is not None and 0.9 < r["traffic"] / (r["algorithmic_bytes_per_step"] * (1 << 20) * 20) < 1.25, r["traffic"]
    assert len(r["kernel_ms_by_rank"]) == 1
    lay = d["layouts"]
    assert set(lay) == {"columns", "blocked", "packed", "narrow", "packed_plus_decode"} and lay["packed"]["headline"] is True
    assert lay["columns"]["kernel"] == "steps_quad_kernel<RockEnv<1>>" and lay["blocked"]["kernel"] == "steps_quad_kernel<RockEnv<1>, Blocked>"
    for k in ("columns", "blocked"):
        assert lay[k]["value"] > 1e8 and 0.3 < lay[k]["roofline"]["hbm_frac"] < 1.0 and lay[k]["kernel_ms"] < 3.6e-3, lay[k]
    assert lay["packed"]["kernel_ms"] < min(lay["columns"]["kernel_ms"], lay["blocked"]["kernel_ms"])
    assert lay["narrow"]["kernel"] == "steps_quad_kernel<RockEnv<1>, Narrow>" and lay["narrow"]["kernel_ms"] < 1.3 * lay["packed"]["kernel_ms"]
    pd = lay["packed_plus_decode"]      # records -> int32 columns costs more than writing the columns in the first place
    assert pd["kernel_ms"] > lay["columns"]["kernel_ms"] and 0.4 < pd["decode_hbm_frac"] < 1.0 and abs(pd["bytes_per_lane_step"] - 21.4) < 1e-9, pd
    cfg = d["configs"]
    assert set(cfg) == {"tag", "battleship", "rollout_rock15", "plan_rock15", "tape_packed", "tape_returns", "returns_only"}
    # the caller's actions instead of the synthetic policy's: the same loops, one load per quad-step instead of one Philox block
    assert cfg["tape_packed"]["kernel"] == "steps_quad_kernel<RockEnv<1>, Packed, Tape>" and cfg["tape_packed"]["invalid_actions"] == 0
    assert cfg["tape_returns"]["kernel"] == "steps_quad_kernel<RockEnv<1>, Returns, Tape>"
    assert cfg["tape_returns"]["kernel_ms"] < 1.15 * cfg["returns_only"]["kernel_ms"], (cfg["tape_returns"], cfg["returns_only"])
    # ... measured against the synthetic policy under the same protocol (same env, sink and regions): recorded 0.97 - 1.06; the
    # bound leaves room for a slow box
    for c in ("tape_packed", "tape_returns"):
        assert 0.7 < cfg[c]["vs_synthetic"] < 1.2 and abs(cfg[c]["vs_synthetic"] - cfg[c]["kernel_ms"] / cfg[c]["synthetic_kernel_ms"]) < 1e-9, cfg[c]
    pl = cfg.pop("plan_rock15")          # configs[4] as planned REAL steps: rollout + on-device reduction + the roots' step
    assert pl["unit"] == "planned real env-steps/s" and pl["value"] > 1e5 and abs(sum(pl["share"].values()) - 1.0) < 1e-6, pl
    assert pl["share"]["rollout"] > 0.8 and pl["reduce_kernel_ms"] < 0.2 and pl["visited_actions_per_root"] > 3, pl
    assert cfg["returns_only"]["kernel"] == "steps_quad_kernel<RockEnv<1>, Returns>" and cfg["returns_only"]["steps_per_launch"] == 256
    assert cfg["tag"]["kernel"].startswith("tag_steps_quad_kernel<true") and cfg["battleship"]["kernel"].startswith("battleship_steps_quad_kernel<BattleShipEnv<4>")
    for k in cfg:
        assert cfg[k]["value"] > 1e10 and cfg[k]["kernel_ms"] > 0 and "frac" in cfg[k]["roofline"], (k, cfg[k])
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "usable_cpus", "kind", "sample", "by_threads"):
        assert k in c, k
    assert c["cores"] == max(c["by_threads"], key=lambda t: t["value"])["threads"] and c["value"] > 1e6 and c["usable_cpus"] >= 1
    assert d["value"] > 1e8          # the north star's single-GPU target, by a wide margin


@pytest.mark.parametrize("mode,env,extra", [("rollout", "rock15", ["--lanes-per-gpu", 2097152, "--steps", 10, "--warmup", 5]),
                                            ("heuristic", "tag", ["--steps", 128, "--warmup", 64, "--prewarm", 0.5])],
                         ids=["rollout-c5", "heuristic-tag"])
def test_compute_bound_modes_report_a_valu_roofline(mode, env, extra):
    """the fused rollout (configs[4]) and the heuristic-policy loop are bound by instruction issue, not by
    bytes: their line's roofline is VALU issue — recorded instructions per launch / the launch time of this run, against
    the SIMDs' issue cycles priced with the kernel's instruction mix — with frac <= 1, and the HBM figure beside it."""
    d = _bench("--env", env, "--mode", mode, *extra)
    r = d["roofline"]
    assert r["bound"] == "valu" and r["unit"] == "wave-instructions/s", r
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.2 < r["frac"] <= 1.0, r
    assert r["hbm"]["bound"] == "hbm" and r["hbm"]["frac"] < 0.5
    assert "profiles/" in r["source"] and d["value"] > 1e10


def test_bench_self_launches_two_ranks_on_the_one_gpu():
    """`python bench.py --gpus 2` (no torch.distributed.run around it) starts its two ranks itself; with one visible GPU
    they share it.  The shards tile the global lane range, the line reports both scaling modes."""
    d = _bench("--gpus", 2, "--share-gpus", "--steps", 64, "--warmup", 5, "--seeds", "0", "--repeats", 5)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    cfg = d["config"]
    assert cfg["lanes_per_gpu"] == 1 << 20 and cfg["total_lanes"] == 2 << 20
    sh = sorted(cfg["shards"], key=lambda s: s["rank"])
    assert [s["rank"] for s in sh] == [0, 1]
    assert sh[0]["lane_offset"] == 0 and sh[1]["lane_offset"] == sh[0]["lanes"] == 1 << 20 and sh[1]["lanes"] == 1 << 20
    assert d["value"] > 1e8 and "cpu_baseline" not in d
    s = d["strong_scaling"]
    assert s["total_lanes"] == 1 << 20 and s["lanes_per_gpu"] == 1 << 19 and s["value"] > 1e8
    # Both ranks share this one GPU, so the two figures are how two processes' launches interleave on a device, not what a
    # GPU per rank gives.  Round 3 (13 B per lane-step, store-bound at 2^20 lanes): 0.87-1.05.  Round 4 (packed records,
    # issue-bound): a 2^19-lane shard runs 1.12 us per step against 1.54 for 2^20 lanes (profiles/r04*_small_shards*.txt), so two
    # of them deliver ~0.7 of what two 2^20-lane shards do
    # (how two PROCESSES' launches interleave on one device varies from run to run — 0.5-0.8 observed; the bound only guards
    # against a shard that runs at a fraction of its speed)
    assert s["value"] > 0.3 * d["value"], (s["value"], d["value"])
    assert len(d["roofline"]["kernel_ms_by_rank"]) == 2


def test_launcher_picks_the_documented_kernel_per_shard_size():
    """pomdp_last_fused_kernel() after a fused call: the quad-per-thread loops from the shard sizes DESIGN.md §5 lists
    (RockSample 3 * 2^18, StochasticRock 2^19, Tag 2^19, Tiger 2^19, Network 2^19, BattleShip 2^16), the one- / two-lanes-per-thread
    loops below, and the arithmetic lane step for launches shorter than 16 steps."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    want = [("rock", {}, 1 << 20, 64, "steps_quad_kernel<RockEnv<1>>"), ("rock", {}, 3 << 18, 64, "steps_quad_kernel<RockEnv<1>>"),
            ("rock", {}, 1 << 19, 64, "steps_kernel<RockEnv<1>, 2, true>"),
            ("rock", {}, 1 << 18, 64, "steps_kernel<RockEnv<1>, 1, true, true>"), ("rock", {}, (1 << 19) + 2048, 8, "steps_kernel<RockEnv<1>, 2, true>"), ("rock", {}, 1 << 17, 64, "steps_kernel<RockEnv<1>, 1, true, true>"), ("rock", {}, 1 << 17, 8, "steps_kernel<RockEnv<1>, 1, true>"),
            ("rock", {}, 1 << 20, 5, "steps_kernel<RockEnv<1>, 4, true>"), ("rock", dict(board_size=15, num_rocks=15), 1 << 20, 64, "steps_quad_kernel<RockEnv<2>>"),
            ("rock", {}, (1 << 19) + 4, 64, "steps_kernel<RockEnv<1>, 2, false>"),
            ("tag", {}, 1 << 19, 64, "tag_steps_quad_kernel<true>"), ("tag", {}, 1 << 19, 8, "tag_steps_quad_kernel<false>"),
            ("tag", {}, 1 << 18, 64, "steps_kernel<TagEnv, 1, true>"), ("tag", dict(num_opponents=2), 1 << 20, 64, "steps_kernel<TagEnv, 2, true>"),
            ("tiger", {}, 1 << 19, 64, "steps_quad_generic_kernel<TigerEnv>"), ("tiger", {}, 1 << 18, 64, "steps_kernel<TigerEnv, 1, true>"),
            ("network", {}, 1 << 19, 64, "network_steps_quad_kernel<2, Columns, true>"), ("network", dict(n_machines=16, problem_type=1), 1 << 19, 64, "network_steps_quad_kernel<2, Columns, false>"), ("network", {}, 1 << 18, 64, "steps_kernel<NetworkEnv, 1, true>"),
            ("battleship", {}, 1 << 16, 64, "battleship_steps_quad_kernel<BattleShipEnv<1>>"), ("battleship", {}, 1 << 15, 64, "steps_kernel<BattleShipEnv<1>, 1, true>"), ("stochrock", {}, 1 << 19, 64, "steps_quad_kernel<StochasticRockEnv<1>>"),
            ("stochrock", {}, 1 << 18, 64, "steps_kernel<StochasticRockEnv<1>, 1, true>")]
    for env, kw, n, k, name in want:
        e = make_env(env, kw, batch_size=n, seed=1, reuse_buffers=True)
        e.reset()
        e.collect_synthetic(k)
        assert L.pomdp_last_fused_kernel().decode() == name, (env, kw, n, k, L.pomdp_last_fused_kernel())
        del e


def test_bound_argument_entry_points_equal_the_plain_ones():
    """pomdp_step / pomdp_collect (arguments bound once in a struct) launch what pomdp_<env>_step / pomdp_collect_synthetic
    launch: same outputs, same state — through the Python mirror's two paths (reuse_buffers=True takes the bound ones)."""
    for env, kw in (("rock", {}), ("tag", {}), ("battleship", {}), ("tiger", {}), ("network", {})):
        a = make_env(env, kw, batch_size=8192, seed=5, lane_offset=16, reuse_buffers=True)      # pomdp_step
        b = make_env(env, kw, batch_size=8192, seed=5, lane_offset=16, reuse_buffers=False)     # pomdp_<env>_step
        assert torch.equal(a.reset(), b.reset())
        for _ in range(6):
            act = b.synthetic_actions()
            ra, rb = a.step(act), b.step(act)
            assert all(torch.equal(x, y) for x, y in zip(ra[:3], rb[:3])) and torch.equal(a.state, b.state), env
        a.auto_reset = False                      # the bound flags follow the attribute
        b.auto_reset = False
        for _ in range(4):
            act = b.synthetic_actions()
            ra, rb = a.step(act), b.step(act)
            assert all(torch.equal(x, y) for x, y in zip(ra[:3], rb[:3])) and torch.equal(a.state, b.state), env


def _heuristic_fused_vs_oracle(oracle_lib, env, kw, n, ks, seed, lane0, max_size=None, auto=True, preset=None, t0=0):
    """The launches `bench.py --mode heuristic` times — heuristic_steps_kernel, up to 64 steps each — against the oracle's
    lane-major restatement of the reference's rollout loop (rock.py:557-573; or_batch_heuristic_steps, pinned on CPU to the
    per-step batch functions the heur_* fixtures pin to the reference): after every launch the outputs it leaves (the LAST
    step's action / ob / reward / done — the fused loop overwrites one row), the state, prev_ob, the history words and
    sums and, for RockSample, the float64 side statistics bit for bit and the two derived words."""
    from gym_pomdp_amd import History
    ol = oracle_lib
    nt = ol.max_threads()
    is_rock = env in ("rock", "stochrock")
    o = ol.OracleEnv(env, **kw)
    e = make_env(env, dict(kw, **(dict(use_heuristic=True) if is_rock else {})), batch_size=n, seed=seed, lane_offset=lane0,
                 auto_reset=auto, reuse_buffers=True)
    st = o.new_state(n)
    e.call_counter = t0                                                  # reset() is call t0, the first step call t0 + 1
    prev = o.batch_reset(st, seed, lane0, t0, nthreads=nt).astype(np.int32)
    assert np.array_equal(np_(e.reset()), prev)
    h = History(e, max_size=max_size)
    b = ol.Belief(o, n) if is_rock else None
    hs = ol.HistorySums(o, n, max_size=max_size)
    frozen = np.zeros(n, np.uint8)
    t, n_done = t0 + 1, 0
    if preset is not None:
        preset(e, h, b, hs)
    for k in ks:
        fa, fo, fr, fd = e.heuristic_steps(h, k)
        want = o.batch_heuristic_steps(st, hs, b, prev, k, seed, lane0, t, auto_reset=auto, done_in=frozen, nthreads=nt)
        t += k
        ctx = (env, kw, n, k, t)
        assert np.array_equal(np_(fa), want["action"][-1]), ctx
        assert np.array_equal(np_(fo), want["ob"][-1]) and np.array_equal(np_(fr), want["reward"][-1]), ctx
        assert np.array_equal(np_(fd), want["done"][-1].astype(bool)), ctx
        assert np.array_equal(np_(e.state).view(np.uint32), st), ctx
        if not auto:
            frozen = want["done"][-1].copy()
        live = frozen == 0
        assert np.array_equal(np_(h.prev_ob)[live], prev[live]), ctx
        # a bounded history's sums are its window's: the oracle keeps the records (rock.py:533-544) and walks them
        ws = dict(zip(("total_sample", "total_move"), hw.window_sums(hs, o.n_actions - 5))) if is_rock and max_size is not None else {}
        for name in ("size", "last_action", "last_ob") + (("total_sample", "total_move") if is_rock else ()):
            got = np_(getattr(h, "_size" if name == "size" else name))
            assert np.array_equal(got[..., live], ws.get(name, getattr(hs, name))[..., live]), ctx + (name,)
        if is_rock:
            gb = {k_: np_(v) for k_, v in e.belief.items()}
            for k_, _ in ol.Belief.FIELDS:
                x, y = gb[k_], getattr(b, k_)
                same = (x.view(np.uint64) == y.view(np.uint64)) if x.dtype == np.float64 else (x == y)
                assert (same | ((x != x) & (y != y))).all(), ctx + (k_,)
            K = o.n_actions - 5
            w = (1 << np.arange(K, dtype=np.int64))[:, None]
            ok = (b.measured < 5) & (np.abs(b.count) < 2) & (b.prob_valuable > 0) & (b.prob_valuable < 1)
            assert np.array_equal((ok * w).sum(axis=0), np_(e._tracker.check_ok).astype(np.int64) & 0xFFFFFFFF), ctx
            mo = np_(h.move_ok).astype(np.int64) & 0xFFFFFFFF
            tm, ts = ws.get("total_move", hs.total_move), ws.get("total_sample", hs.total_sample)
            assert np.array_equal(((tm >= 0) * w).sum(axis=0), mo & 0xFFFF), ctx
            assert np.array_equal(((ts > 0) * w).sum(axis=0), mo >> 16), ctx
            if max_size is not None:                                     # the ring read back as records == the oracle's records
                W = max_size + 1
                win = hw.decode_ring(np_(h.ring), np_(h.head), np_(h._size), W)
                v = (np.arange(W)[:, None] < hs.size[None, :]) & live[None, :]
                assert np.array_equal(win["valid"][:, live], (np.arange(W)[:, None] < hs.size[None, :])[:, live]), ctx
                for name, rec in (("action", hs.rec[1]), ("next", hs.rec[2]), ("bad", hs.rec[0] == 1)):
                    assert np.array_equal(win[name][v], rec[v]), ctx + ("ring", name)
        n_done += int(want["done"].sum())
    return n_done


@pytest.mark.parametrize("env,kw", [("rock", {}), ("rock", dict(board_size=15, num_rocks=15)), ("tag", {})],
                         ids=["rock_7_8", "rock_15_15", "tag"])
def test_heuristic_steps_fused_vs_oracle(oracle_lib, env, kw):
    """2^20 lanes, heuristic_steps(h, 64) twice (then a short launch that ends off a multiple of four steps)."""
    n_done = _heuristic_fused_vs_oracle(oracle_lib, env, kw, 1 << 20, (64, 64, 7), seed=0xBEEF, lane0=1 << 21)
    assert n_done > 0


@pytest.mark.parametrize("env,kw,n,max_size,auto", [("rock", {}, 4096 + 1, None, True), ("rock", {}, 4096 + 2, 6, True),
                                                    ("rock", dict(board_size=15, num_rocks=15), 2048 + 3, None, True),
                                                    ("tag", {}, 4096 + 3, None, True), ("stochrock", {}, 1024 + 1, None, False),
                                                    ("tiger", {}, 259, None, True), ("battleship", {}, 1021, None, True),
                                                    ("rock", {}, 2048, 80, True), ("rock", {}, 4096 + 2, 0, True),
                                                    ("rock", {}, 4096 + 2, 1, True), ("rock", {}, 4096 + 2, 3, True)],
                         ids=["rock+1", "rock+2-hist6", "rock15+3", "tag+3", "stochrock+1-frozen", "tiger+3", "battleship+1", "rock-hist80",
                              "rock+2-hist0", "rock+2-hist1", "rock+2-hist3"])
def test_heuristic_multi_step_launches_on_ragged_batches_vs_oracle(oracle_lib, env, kw, n, max_size, auto):
    """n % 4 != 0 with several steps per launch: the padding threads of the last quad take part in the quad transposes that
    hand the policy's (and RockSample's sensor) blocks of steps base + 1 .. 3 to the quad's in-range lanes, so their lane
    ids must be the unclamped ones (round 3's advisor finding: they used lane n - 1's).  hist0 / hist1 / hist3: windows
    shorter than the step loop's unroll of four, carried in registers across the launch."""
    _heuristic_fused_vs_oracle(oracle_lib, env, kw, n, (64, 5, 64, 2), seed=4242, lane0=1 << 10, max_size=max_size, auto=auto)


def test_heuristic_loop_over_many_launches_with_lanes_that_keep_checking(oracle_lib):
    """RockSample(15,15) past the phase in which the rocks get measured: most lanes never CHECK again, one in 500 stands on a
    rock it cannot decide about and CHECKs in three steps of four (the legal fallback of rock.py:374: ~190 CHECKs per 256
    steps, `measured` far past 5) — every array after every launch.  1 280 steps, six launches."""
    n_done = _heuristic_fused_vs_oracle(oracle_lib, "rock", dict(board_size=15, num_rocks=15), 8192 + 3, (256, 256, 256, 256, 255, 1),
                                        seed=77, lane0=12)
    assert n_done > 0


@pytest.mark.parametrize("env,kw,max_size", [("rock", dict(board_size=15, num_rocks=15), None), ("rock", {}, None), ("rock", {}, 9),
                                             ("stochrock", {}, None)], ids=["rock15", "rock", "rock-hist9", "stochrock"])
def test_heuristic_loop_from_statistics_far_from_fresh(oracle_lib, env, kw, max_size):
    """The heuristic loop started from statistics far from a fresh episode's: sums and counts of thousands either sign, rocks
    measured hundreds of times, rocks whose prob_valuable is already closed (a likelihood of exactly 0) — every array, bit
    for bit, after every launch (a loop that kept narrow copies of them, docs/HISTORY.md §A round 5, was checked with these)."""
    def preset(e, h, b, hs):
        K, n = b.count.shape
        rng = np.random.default_rng(5)
        edge = np.array([-70000, -2049, -2048, -2047, -2046, -300, -2, -1, 0, 0, 0, 1, 2, 300, 2046, 2047, 2048, 2049, 70000], np.int32)
        hs.total_sample[:] = rng.choice(edge, size=(K, n))
        hs.total_move[:] = rng.choice(edge, size=(K, n))
        far = rng.random((K, n)) < .3                                    # rocks measured out long ago
        b.measured[:] = np.where(far, rng.choice(np.array([5, 14, 15, 16, 250, 70000]), size=(K, n)), rng.integers(0, 5, size=(K, n)))
        b.count[:] = np.where(far, rng.choice(np.array([-130, -9, -8, -7, -6, 6, 7, 8, 9, 130]), size=(K, n)),
                              rng.integers(-2, 3, size=(K, n)))
        closed = rng.random((K, n)) < .2                                 # a CHECK from distance 0 came first
        b.lkw[:] = np.where(closed, 0., 1.)
        b.prob_valuable[:] = np.where(closed, 1., .5)
        if max_size is None:                                             # (a bounded history's sums are its window's: left at 0)
            h.total_sample.copy_(torch.as_tensor(hs.total_sample)); h.total_move.copy_(torch.as_tensor(hs.total_move))
            w = (1 << np.arange(K, dtype=np.int64))[:, None]
            mo = ((hs.total_move >= 0) * w).sum(axis=0) | (((hs.total_sample > 0) * w).sum(axis=0) << 16)
            h.move_ok.copy_(torch.as_tensor(mo.astype(np.uint32).view(np.int32)))
        else:
            hs.total_sample[:] = 0; hs.total_move[:] = 0
        e.set_belief({k_: torch.as_tensor(getattr(b, k_)) for k_, _ in type(b).FIELDS})
    _heuristic_fused_vs_oracle(oracle_lib, env, kw, 4096 + 1, (64, 256, 7), seed=99, lane0=8, max_size=max_size, preset=preset)


# ---- the single-stream trajectory layouts (include/pomdp_hip.h: POMDP_LAYOUT_BLOCKED / _PACKED; csrc/traj_out.hip.h) --------
LAYOUT_FULL = [("rock", {}, 1 << 20, 70), ("rock", {}, 1 << 20, 20), ("rock", dict(board_size=15, num_rocks=15), 1 << 20, 66),
               ("rock", dict(board_size=4, num_rocks=3), 1 << 20, 40), ("stochrock", {}, 1 << 19, 70), ("tag", {}, 1 << 20, 70),
               ("tag", dict(num_opponents=3), 1 << 20, 40), ("tiger", {}, 1 << 20, 70), ("network", {}, 1 << 20, 70),
               ("network", dict(n_machines=31, problem_type=3), 1 << 19, 40),
               ("battleship", dict(board_size=(10, 10), max_len=5), 1 << 19, 70), ("battleship", {}, 1 << 20, 130),
               # the shards a 2^20-lane batch leaves per GPU at 2 / 4 / 8 GPUs (the one- and two-lanes-per-thread loops)
               ("rock", {}, 1 << 19, 66), ("rock", {}, 1 << 18, 66), ("rock", {}, 1 << 17, 66), ("tag", {}, 1 << 18, 66),
               ("tiger", {}, 1 << 17, 66), ("network", {}, 1 << 18, 66), ("battleship", {}, 1 << 17, 66),
               # ragged batches: rows padded to the layout's pitch, the general (not SIMPLE) loop
               ("rock", {}, 4099, 70), ("tag", {}, (1 << 18) + 5, 20), ("network", {}, 777, 70), ("tiger", {}, 3, 70),
               ("battleship", {}, 259, 70), ("rock", dict(board_size=15, num_rocks=15), (1 << 19) + 4, 30),
               # RockSample's half-quad-per-thread loop (above 3 * 2^17, below 3 * 2^18 lanes; 2^19 is above) and StochasticRock's
               # (3 * 2^17 .. 2^19 - 1)
               ("rock", {}, 7 << 16, 40), ("rock", dict(board_size=15, num_rocks=15), 5 << 17, 40), ("rock", {}, (3 << 18) - 1024, 20),
               ("stochrock", dict(board_size=11, num_rocks=11), 3 << 17, 30), ("stochrock", {}, (1 << 19) - 1024, 40),
               # Tag's (3 * 2^17 .. 3 * 2^18 - 1 lanes)
               ("tag", {}, 1 << 19, 66), ("tag", dict(move_prob=0.4), 5 << 17, 40), ("tag", {}, 3 << 17, 40), ("tag", {}, (3 << 18) - 1024, 20)]


LAYOUTS = ("blocked", "packed", "narrow")


@pytest.mark.parametrize("env,kw,n,steps", LAYOUT_FULL, ids=["%s%s-%d-%d" % (c[0], "-".join(str(v) for v in c[1].values()), c[2], c[3]) for c in LAYOUT_FULL])
def test_single_stream_layouts_equal_the_oracle(oracle_lib, env, kw, n, steps):
    """collect_synthetic(steps, layout=...) — the blocked (13 B per lane-step, int32 / float values, one contiguous block
    per wave-step), packed (one 32-bit record per lane-step, decoded by pomdp_decode_packed) and narrow (the record's bytes
    as four typed planes) trajectories — compared with the oracle row by row over the whole batch, then the state: the same
    information as the four columns of the default ABI (rock.py:553-575: `ob, rw, done, info = env.step(action)` per
    step).  One oracle pass per case; one env per layout, all on the same seed."""
    seed, lane0, t0 = 20260930, 1 << 22, (1 << 33) + 9
    nt = oracle_lib.max_threads()
    o = oracle_lib.OracleEnv(env, **kw)
    st = o.new_state(n)
    ob0 = o.batch_reset(st, seed, lane0, t0, nthreads=nt)
    envs, decs = {}, {}
    for layout in LAYOUTS:
        e = envs[layout] = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
        e.call_counter = t0
        assert np.array_equal(np_(e.reset()), ob0)
        tr = e.collect_synthetic(steps, layout=layout)
        assert tr["layout"] == layout and e.call_counter == t0 + 1 + steps and "layout" not in e.trajectory_buffers(1)
        decs[layout] = e.decode_trajectory(tr)
    done = np.zeros(n, np.uint8)
    for k in range(steps):
        t = t0 + 1 + k
        a = oracle_lib.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt)
        ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
        assert bad == 0, (env, kw, n, k)
        for layout in LAYOUTS:
            dec, ctx = decs[layout], (env, kw, n, k, layout)
            assert np.array_equal(np_(dec["action"][k]), a), ctx
            assert np.array_equal(np_(dec["ob"][k]), ob), ctx
            got_r = np_(dec["reward"][k])
            # narrow: the reward plane is the int8 reward itself (Network: gathered through the table, float32)
            assert got_r.dtype == (np.int8 if layout == "narrow" and env != "network" else rew.dtype) and np.array_equal(got_r, rew), ctx
            assert np.array_equal(np_(dec["done"][k]), done.astype(bool)), ctx
    for layout in LAYOUTS:
        assert np.array_equal(np_(envs[layout].state).view(np.uint32), st), layout
        assert envs[layout].invalid_action_count() == 0
    # the next call continues the same trajectory (it derives its first actions from (seed, lane, t) again)
    d2 = {layout: envs[layout].decode_trajectory(envs[layout].collect_synthetic(3, layout=layout)) for layout in LAYOUTS}
    for k in range(3):
        t = t0 + 1 + steps + k
        a = oracle_lib.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt)
        ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
        for layout in LAYOUTS:
            d = d2[layout]
            assert np.array_equal(np_(d["action"][k]), a) and np.array_equal(np_(d["ob"][k]), ob) and np.array_equal(np_(d["reward"][k]), rew), layout
    for layout in LAYOUTS:
        assert np.array_equal(np_(envs[layout].state).view(np.uint32), st), layout


def test_layout_kernels_are_the_quad_loops_with_another_sink():
    """pomdp_last_fused_kernel() names the layout the launch wrote (as a profiler shows the template argument)."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    want = [("rock", {}, 1 << 20, 64, "packed", "steps_quad_kernel<RockEnv<1>, Packed>"),
            ("rock", {}, 1 << 20, 64, "blocked", "steps_quad_kernel<RockEnv<1>, Blocked>"),
            ("rock", {}, 1 << 18, 64, "packed", "steps_kernel<RockEnv<1>, 1, true, true, Packed>"),
            ("rock", {}, 1 << 19, 64, "blocked", "steps_kernel<RockEnv<1>, 2, true, false, Blocked>"),
            ("tag", {}, 1 << 20, 64, "packed", "tag_steps_quad_kernel<true, Packed>"),
            ("tiger", {}, 1 << 20, 64, "blocked", "steps_quad_generic_kernel<TigerEnv, Blocked>"),
            ("network", {}, 1 << 20, 64, "packed", "network_steps_quad_kernel<2, Packed, true>"),
            ("rock", {}, 1 << 20, 64, "narrow", "steps_quad_kernel<RockEnv<1>, Narrow>"), ("tag", {}, 1 << 18, 64, "narrow", "steps_kernel<TagEnv, 1, true, false, Narrow>"),
            ("battleship", {}, 1 << 18, 64, "packed", "battleship_steps_quad_kernel<BattleShipEnv<1>, Packed, 2>"),
            ("rock", {}, 1 << 19, 64, "packed", "steps_quad_kernel<RockEnv<1>, Packed, 2>"), ("rock", {}, 3 << 17, 64, "narrow", "steps_kernel<RockEnv<1>, 1, true, true, Narrow>"),
            ("rock", {}, (3 << 17) + 1024, 64, "narrow", "steps_quad_kernel<RockEnv<1>, Narrow, 2>"), ("rock", {}, 3 << 18, 64, "packed", "steps_quad_kernel<RockEnv<1>, Packed>"),
            ("rock", dict(board_size=15, num_rocks=15), 5 << 17, 64, "narrow", "steps_quad_kernel<RockEnv<2>, Narrow, 2>"), ("rock", {}, 1 << 19, 8, "packed", "steps_kernel<RockEnv<1>, 2, true, false, Packed>"),
            ("tag", {}, 1 << 19, 64, "packed", "tag_steps_quad_kernel<true, Packed, 2>"), ("tag", {}, 1 << 19, 8, "packed", "tag_steps_quad_kernel<false, Packed>"),
            ("tag", {}, 3 << 18, 64, "narrow", "tag_steps_quad_kernel<true, Narrow>"), ("tag", {}, 3 << 17, 64, "narrow", "tag_steps_quad_kernel<true, Narrow, 2>"),
            ("tag", {}, 1 << 19, 64, "blocked", "tag_steps_quad_kernel<true, Blocked>"),
            ("stochrock", {}, 1 << 19, 64, "packed", "steps_quad_kernel<StochasticRockEnv<1>, Packed>"), ("stochrock", {}, 3 << 17, 64, "packed", "steps_quad_kernel<StochasticRockEnv<1>, Packed, 2>"),
            ("tiger", {}, 1000, 64, "packed", "steps_kernel<TigerEnv, 1, false, false, Packed>")]
    for env, kw, n, k, layout, name in want:
        e = make_env(env, kw, batch_size=n, seed=1, reuse_buffers=True)
        e.reset()
        e.collect_synthetic(k, layout=layout)
        assert L.pomdp_last_fused_kernel().decode() == name, (env, kw, n, k, layout, L.pomdp_last_fused_kernel())
        del e


def test_collect_layout_through_the_c_abi():
    """pomdp_collect_layout called directly: a row pitch larger than n in both layouts (the padding is never written),
    equality with the column layout's values, and the argument checks."""
    import ctypes as C
    from gym_pomdp_amd import _native
    L = _native.lib()
    n, steps, seed = 5000, 67, 77
    ref = make_env("rock", {}, batch_size=n, seed=seed, lane_offset=8, reuse_buffers=True)
    ref.reset()
    cols = ref.collect_synthetic(steps)
    s = torch.cuda.current_stream().cuda_stream
    for layout, pitch, row, dt in ((1, 5120, 5120 * 13, torch.uint8), (2, 5008, 5008, torch.int32)):
        e = make_env("rock", {}, batch_size=n, seed=seed, lane_offset=8, reuse_buffers=True)
        e.reset()
        traj = torch.full((steps, row), 0x5A if layout == 1 else 0x5A5A5A5A, dtype=dt, device="cuda")
        rc = L.pomdp_collect_layout(_native.ENV_KIND["rock"], C.byref(e._params), e._state.data_ptr(), traj.data_ptr(), e._err.data_ptr(),
                                    n, seed, 8, e.call_counter, steps, pitch, layout, _native.POMDP_AUTO_RESET, s)
        assert rc == 0
        torch.cuda.synchronize()
        d = e.decode_trajectory({"layout": "blocked" if layout == 1 else "packed", "pitch": pitch, "traj": traj})
        assert torch.equal(d["action"], cols["action"][:steps]) and torch.equal(d["ob"], cols["ob"])
        assert torch.equal(d["reward"], cols["reward"]) and torch.equal(d["done"], cols["done"])
        assert torch.equal(e.state, ref.state)
        if layout == 2:                                     # the padding lanes of every row are untouched
            assert bool((traj[:, n:] == 0x5A5A5A5A).all())
        else:
            blocks = traj.view(steps, pitch // 256, 13 * 256)
            assert bool((blocks[:, -1, 4 * (n % 256):1024] == 0x5A).all()) and bool((blocks[:, -1, 3072 + n % 256:] == 0x5A).all())
        bad = lambda *a: L.pomdp_collect_layout(*a)        # noqa: E731
        args = [_native.ENV_KIND["rock"], C.byref(e._params), e._state.data_ptr(), traj.data_ptr(), e._err.data_ptr(), n, seed, 8, 0, 4, pitch,
                layout, _native.POMDP_AUTO_RESET, s]
        assert bad(*args[:11], 0, *args[12:]) == -1         # POMDP_LAYOUT_COLUMNS has its own entry point
        assert bad(*args[:12], 0, s) == -1                  # auto-reset is required
        assert bad(*args[:10], n - 1, *args[11:]) == -1     # pitch < n
        if layout == 1:
            assert bad(*args[:10], pitch + 4, *args[11:]) == -1   # blocked rows are whole 256-lane blocks
    t = make_env("tag", dict(obs_cells=300), batch_size=1024, seed=1, reuse_buffers=True)
    t.reset()
    with pytest.raises(RuntimeError):
        t.collect_synthetic(4, layout="packed")             # "opponent seen" = 300 does not fit the record's ob byte
    t.collect_synthetic(4, layout="blocked")
    assert L.pomdp_packed_reward(_native.ENV_KIND["rock"], 0x9C) == -100.0 and L.pomdp_packed_reward(_native.ENV_KIND["network"], 68 + 7) == float(np.float32(6.9))


# ---- the returns-only sink (include/pomdp_hip.h: pomdp_collect_returns; csrc/traj_out.hip.h: Returns) -----------------------
RETURNS_FULL = [("rock", {}, 1 << 20, (70, 20)), ("rock", dict(board_size=15, num_rocks=15), 1 << 20, (66, 3)), ("tag", {}, 1 << 20, (70, 5)),
                ("tiger", {}, 1 << 20, (70, 5)), ("network", {}, 1 << 20, (70, 5)),
                ("battleship", dict(board_size=(10, 10), max_len=5), 1 << 19, (70, 5)), ("battleship", {}, 1 << 20, (130, 7)),
                ("stochrock", {}, 1 << 19, (40, 30)), ("tag", dict(num_opponents=3), 1 << 20, (40, 3)),
                ("network", dict(n_machines=31, problem_type=3), 1 << 19, (40, 3)),
                # the shards a 2^20-lane batch leaves per GPU (the one- and two-lanes-per-thread loops) and ragged batches
                ("rock", {}, 1 << 19, (66, 4)), ("rock", {}, 1 << 18, (66, 4)), ("rock", {}, 1 << 17, (66, 4)), ("tag", {}, 1 << 18, (66, 4)),
                ("tiger", {}, 1 << 17, (66, 4)), ("network", {}, 1 << 18, (66, 4)), ("battleship", {}, 1 << 17, (66, 4)),
                ("rock", {}, 4099, (70, 9)), ("tag", {}, (1 << 18) + 5, (20, 9)), ("network", {}, 777, (70, 9)), ("tiger", {}, 3, (70, 9)),
                ("battleship", {}, 259, (70, 9)), ("rock", dict(board_size=15, num_rocks=15), (1 << 19) + 4, (30, 9)),
                ("rock", dict(board_size=15, num_rocks=15), 5 << 17, (40, 9)), ("stochrock", {}, 7 << 16, (30, 9)),   # between the gates
                ("tag", {}, 1 << 19, (66, 4)), ("tag", {}, 3 << 17, (40, 9))]


@pytest.mark.parametrize("env,kw,n,ks", RETURNS_FULL, ids=["%s%s-%d" % (c[0], "-".join(str(v) for v in c[1].values()), c[2]) for c in RETURNS_FULL])
def test_collected_returns_equal_the_oracle(oracle_lib, env, kw, n, ks):
    """collect_returns(k) — the fused launches with the Returns sink: nothing written per step, per lane the reference
    callers' reduction `r += discount * rw; discount *= .95`, one return per episode (network.py:175-191, rock.py:553-575) —
    against the oracle's lane-major restatement: running return and discount, last finished return, the sum over finished
    episodes (float64, bit for bit), episode and step counts, and the state; a second call continues the same statistics."""
    from gym_pomdp_amd import EpisodeStats
    seed, lane0, t0 = 20261001, 1 << 22, (1 << 33) + 11
    nt = oracle_lib.max_threads()
    e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
    e.call_counter = t0
    o = oracle_lib.OracleEnv(env, **kw)
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, t0, nthreads=nt))
    stats = EpisodeStats(e)
    acc, cnt = oracle_lib.new_return_stats(n)
    t, n_done = t0 + 1, 0
    for k in ks:
        assert e.collect_returns(k, stats) is stats
        n_done += o.batch_collect_returns(st, acc, cnt, e._discount, seed, lane0, t, k, nthreads=nt)
        t += k
        ctx = (env, kw, n, k)
        for q, name in enumerate(("ret", "disc", "ret_done", "ret_sum")):
            assert np.array_equal(np_(getattr(stats, name)).view(np.uint64), acc[q].view(np.uint64)), ctx + (name,)
        assert np.array_equal(np_(stats.episodes), cnt[0]) and np.array_equal(np_(stats.steps), cnt[1]), ctx
        assert np.array_equal(np_(e.state).view(np.uint32), st), ctx
    assert e.call_counter == t and e.invalid_action_count() == 0
    if env != "network":
        assert n_done > 0 and int(cnt[0].sum()) == n_done                # Network never terminates (network.py:113)
        assert abs(stats.mean_return() - acc[3].sum() / n_done) < 1e-9 * max(1.0, abs(acc[3].sum() / n_done))
    # the same steps as collect_synthetic: the trajectory's rewards reduce to the same returns
    e2 = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
    e2.call_counter = t0
    e2.reset()
    e2.collect_synthetic(sum(ks))
    assert torch.equal(e2.state, e.state)


def test_returns_kernels_are_the_fused_loops_with_the_returns_sink():
    from gym_pomdp_amd import _native
    L = _native.lib()
    want = [("rock", {}, 1 << 20, "steps_quad_kernel<RockEnv<1>, Returns>"), ("rock", {}, 1 << 17, "steps_kernel<RockEnv<1>, 1, true, true, Returns>"),
            ("tag", {}, 1 << 20, "tag_steps_quad_kernel<true, Returns>"), ("network", {}, 1 << 20, "network_steps_quad_kernel<2, Returns, true>"),
            ("battleship", {}, 1 << 18, "battleship_steps_quad_kernel<BattleShipEnv<1>, Returns, 2>"),
            ("tiger", {}, 1000, "steps_kernel<TigerEnv, 1, false, false, Returns>")]
    for env, kw, n, name in want:
        e = make_env(env, kw, batch_size=n, seed=1, reuse_buffers=True)
        e.reset()
        e.collect_returns(64)
        assert L.pomdp_last_fused_kernel().decode() == name, (env, n, L.pomdp_last_fused_kernel())


def test_collect_returns_through_the_c_abi():
    """pomdp_collect_returns called directly: a pitch larger than n (the padding is never touched), unaligned statistics
    (the general loop), the argument checks."""
    import ctypes as C
    from gym_pomdp_amd import _native
    L = _native.lib()
    n, steps, seed = 5000, 67, 78
    ref = make_env("rock", {}, batch_size=n, seed=seed, lane_offset=8, reuse_buffers=True)
    ref.reset()
    want = ref.collect_returns(steps)
    s = torch.cuda.current_stream().cuda_stream
    for pitch, off in ((5120, 0), (5001, 1)):
        e = make_env("rock", {}, batch_size=n, seed=seed, lane_offset=8, reuse_buffers=True)
        e.reset()
        acc = torch.full((4 * pitch + off,), -7.0, dtype=torch.float64, device="cuda")
        cnt = torch.full((2 * pitch + off,), -7, dtype=torch.int32, device="cuda")
        a, c = acc[off:].view(4, pitch), cnt[off:].view(2, pitch)
        a[:, :n] = 0
        a[1, :n] = 1
        a[2, :n] = float("nan")
        c[:, :n] = 0
        st = _native.ReturnStats(e._discount, a.data_ptr(), c.data_ptr(), pitch)
        args = [_native.ENV_KIND["rock"], C.byref(e._params), e._state.data_ptr(), C.byref(st), e._err.data_ptr(), n, seed, 8,
                e.call_counter, steps, _native.POMDP_AUTO_RESET, s]
        assert L.pomdp_collect_returns(*args) == 0
        torch.cuda.synchronize()
        for q, name in enumerate(("ret", "disc", "ret_done", "ret_sum")):
            assert torch.equal(a[q, :n].view(torch.int64), getattr(want, name).view(torch.int64)), (pitch, name)
        assert torch.equal(c[0, :n], want.episodes) and torch.equal(c[1, :n], want.steps)
        assert bool((a[:, n:] == -7.0).all()) and bool((c[:, n:] == -7).all()) and torch.equal(e.state, ref.state)
        assert L.pomdp_collect_returns(*args[:10], 0, s) == -1          # auto-reset is required
        assert L.pomdp_collect_returns(*args[:3], None, *args[4:]) == -1
        bad = _native.ReturnStats(e._discount, a.data_ptr(), c.data_ptr(), n - 1)
        assert L.pomdp_collect_returns(*args[:3], C.byref(bad), *args[4:]) == -1


def test_decode_packed_through_the_c_abi():
    """pomdp_decode_packed: records -> the default ABI's columns in one device pass.  Every reward code of every env against
    pomdp_packed_reward (the 256 codes as one row of records), a pitch larger than n on both sides (padding untouched), the
    unaligned (scalar) form, and a collected packed trajectory against the column layout's own rows."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    codes = torch.arange(256, dtype=torch.int32, device="cuda")
    rec = (codes & 0xFF) | (((255 - codes) & 0xFF) << 8) | (codes << 16) | ((codes & 1) << 24)
    for env, rdt in (("rock", torch.int32), ("tag", torch.float32), ("battleship", torch.int32), ("tiger", torch.int32), ("network", torch.float32)):
        kind = _native.ENV_KIND[env]
        for off in (0, 1):                                   # 1: nothing is 16-byte aligned -> the scalar form
            a = torch.full((256 + off,), -5, dtype=torch.int32, device="cuda")
            o, d = torch.full_like(a, -5), torch.full((256 + off,), 9, dtype=torch.uint8, device="cuda")
            r = torch.full((256 + off,), -5, dtype=rdt, device="cuda")
            rc = L.pomdp_decode_packed(kind, rec.data_ptr(), 256, 1, 256, a[off:].data_ptr(), o[off:].data_ptr(), r[off:].data_ptr(),
                                       d[off:].data_ptr(), 256, s)
            assert rc == 0
            want = torch.tensor([L.pomdp_packed_reward(kind, c) for c in range(256)], dtype=torch.float64).to(rdt).cuda()
            assert torch.equal(a[off:], codes) and torch.equal(o[off:], 255 - codes) and torch.equal(d[off:], (codes & 1).to(torch.uint8))
            assert torch.equal(r[off:].view(torch.int32), want.view(torch.int32)), (env, off)
    assert L.pomdp_packed_reward(_native.ENV_KIND["tiger"], 0xEC) == -20.0     # tiger.py:165-172 (not -100)
    n, steps, seed = 5000, 67, 79
    for env, kw in (("rock", {}), ("network", {}), ("tag", {})):
        ref = make_env(env, kw, batch_size=n, seed=seed, lane_offset=8, reuse_buffers=True)
        ref.reset()
        cols = ref.collect_synthetic(steps)
        e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=8, reuse_buffers=True)
        e.reset()
        tr = e.collect_synthetic(steps, layout="packed")
        pitch = 5120
        out = [torch.full((steps, pitch), -3, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, cols["reward"].dtype)]
        dn = torch.full((steps, pitch), 7, dtype=torch.uint8, device="cuda")
        rc = L.pomdp_decode_packed(_native.ENV_KIND[env], tr["traj"].data_ptr(), n, steps, tr["pitch"], out[0].data_ptr(), out[1].data_ptr(),
                                   out[2].data_ptr(), dn.data_ptr(), pitch, s)
        assert rc == 0
        assert torch.equal(out[0][:, :n], cols["action"][:steps]) and torch.equal(out[1][:, :n], cols["ob"])
        assert torch.equal(out[2][:, :n], cols["reward"]) and torch.equal(dn[:, :n], cols["done_u8"])
        assert bool((out[0][:, n:] == -3).all()) and bool((out[2][:, n:] == -3).all()) and bool((dn[:, n:] == 7).all())
        d2 = e.decode_trajectory(tr, into=e.trajectory_buffers(steps))
        assert torch.equal(d2["reward"], cols["reward"]) and torch.equal(d2["done"], cols["done"])
    assert L.pomdp_decode_packed(0, None, 4, 1, 4, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), dn.data_ptr(), 4, s) == -1
    assert L.pomdp_decode_packed(0, tr["traj"].data_ptr(), 8, 1, 4, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), dn.data_ptr(), 8, s) == -1


@pytest.mark.parametrize("env,kw,n", [("rock", {}, 1 << 20), ("rock", {}, 1 << 17), ("battleship", {}, 1 << 18), ("tag", {}, 1 << 20),
                                      ("network", {}, 1 << 19), ("tiger", {}, 4099)],
                         ids=["rock", "rock-2e17", "battleship5", "tag", "network", "tiger-ragged"])
def test_launches_longer_than_64_steps(oracle_lib, env, kw, n):
    """pomdp_fuse_max(256): up to 256 steps per fused launch (BattleShip 5x5 plays several episodes per lane inside one) —
    every collected row against the oracle across the new launch boundary, then the statistics of the returns sink, and
    the same rows with the default 64 steps per launch: results never depend on the launch length."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    seed, lane0, steps = 606, 1 << 12, 300
    nt = oracle_lib.max_threads()
    assert L.pomdp_fuse_max(0) == _native.FUSE_MAX_DEFAULT
    try:
        assert L.pomdp_fuse_max(256) == _native.FUSE_MAX_DEFAULT and L.pomdp_fuse_max(1000) == 256 and L.pomdp_fuse_max(0) == 256
        e = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
        o = oracle_lib.OracleEnv(env, **kw)
        st = o.new_state(n)
        assert np.array_equal(np_(e.reset()), o.batch_reset(st, seed, lane0, 0, nthreads=nt))
        tr = e.collect_synthetic(steps, layout="packed")
        dec = e.decode_trajectory(tr)
        done = np.zeros(n, np.uint8)
        for k in range(steps):
            a = oracle_lib.synthetic_actions(n, seed, lane0, 1 + k, o.n_actions, nthreads=nt)
            ob, rew, done, bad = o.batch_step(st, a, seed, lane0, 1 + k, auto_reset=True, done=done, nthreads=nt)
            assert np.array_equal(np_(dec["action"][k]), a) and np.array_equal(np_(dec["ob"][k]), ob), (env, k)
            assert np.array_equal(np_(dec["reward"][k]), rew) and np.array_equal(np_(dec["done"][k]), done.astype(bool)), (env, k)
        assert np.array_equal(np_(e.state).view(np.uint32), st)
        stats = e.collect_returns(steps)
        acc, cnt = oracle_lib.new_return_stats(n)
        o.batch_collect_returns(st, acc, cnt, e._discount, seed, lane0, 1 + steps, steps, nthreads=nt)
        assert np.array_equal(np_(stats.acc[:, :n]).view(np.uint64), acc.view(np.uint64)) and np.array_equal(np_(stats.cnt[:, :n]), cnt)
        assert np.array_equal(np_(e.state).view(np.uint32), st)
        L.pomdp_fuse_max(64)
        e2 = make_env(env, kw, batch_size=n, seed=seed, lane_offset=lane0, reuse_buffers=True)
        e2.reset()
        tr2 = e2.collect_synthetic(steps, layout="packed")
        assert torch.equal(tr2["traj"][:, :n], tr["traj"][:, :n])
    finally:
        L.pomdp_fuse_max(_native.FUSE_MAX_DEFAULT)
