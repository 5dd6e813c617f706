"""RockSample's quad and half-quad loops (steps_quad_kernel) on 16-byte table entries (rock.hip.h: RecWide): the launches a
tape does not reach, and the tape's invalid actions.

With the wide entries the record's action byte comes out of the table — the action only addresses the entry — and the state
word lives in a layout of its own between the launch's load and its store.  Scripted tapes (test_gpu_rock_quad_insert.py) walk
the Tape instantiations; the SyntheticQuad ones, which bench.py times, are walked here: collect_synthetic on the largest and
the smallest board of the form, RockSample(7,8) and (2,1), through every sink the loop has (a quad per thread: packed, columns,
blocked, narrow, returns; half a quad: packed and narrow), every row and the state the launch leaves against the oracle fed the
same synthetic actions — one oracle pass per (env, board, batch), shared by the sinks — and StochasticRock(7,8) with packed
records, where the gate's refusal writes the action into the record from outside the table.

An out-of-range action on a tape looks up entry 0 and is overridden afterwards: its row is (action, 0, 0, 0), the lane's state
stays as it was, and it is counted.

Every launch is 16 steps at the smallest batch the launcher gives the loop."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import make_env, np_

pytestmark = pytest.mark.gpu

STEPS = 16
SEED, LANE0, T0 = 160016, 1 << 21, (1 << 32) + 5
LOOPS = {"rock": {"quad": 3 << 18, "half": (3 << 17) + 4096}, "stochrock": {"quad": 1 << 19, "half": 3 << 17}}
SINKS = {"quad": ("packed", "columns", "blocked", "narrow", "returns"), "half": ("packed", "narrow")}
BOARDS = {"7-8": dict(), "2-1": dict(board_size=2, num_rocks=1)}
ENV_NAME = {"rock": "RockEnv<1>", "stochrock": "StochasticRockEnv<1>"}


def kernel_name(env, layout, loop, tape=False):
    args = [ENV_NAME[env]] + ([] if layout == "columns" else [layout.capitalize()]) + (["Tape"] if tape else []) + (["2"] if loop == "half" else [])
    return "steps_quad_kernel<%s>" % ", ".join(args)


def last_kernel():
    from gym_pomdp_amd import _native
    return _native.lib().pomdp_last_fused_kernel().decode()


@functools.lru_cache(maxsize=None)
def oracle_pass(env, board, n):
    """STEPS synthetic-policy steps of a fresh batch by the oracle -> (rows of (a, ob, reward, done), final state, the
    returns sink's statistics (acc, cnt)); nobody writes to what this returns"""
    from oracle import oracle_lib as ol
    nt = ol.max_threads()
    o = ol.OracleEnv(env, **BOARDS[board])
    st = o.new_state(n)
    ob0 = o.batch_reset(st, SEED, LANE0, T0, nthreads=nt)
    st_r = st.copy()
    done, rows = np.zeros(n, np.uint8), []
    for k in range(STEPS):
        t = T0 + 1 + k
        a = ol.synthetic_actions(n, SEED, LANE0, t, o.n_actions, nthreads=nt)
        ob, rew, done, bad = o.batch_step(st, a, SEED, LANE0, t, auto_reset=True, done=done, nthreads=nt)
        assert bad == 0
        rows.append((a, ob.copy(), rew.copy(), done.copy()))
    acc, cnt = ol.new_return_stats(n)
    o.batch_collect_returns(st_r, acc, cnt, 0.95, SEED, LANE0, T0 + 1, STEPS, nthreads=nt)
    assert np.array_equal(st_r, st)
    return ob0, rows, st, acc, cnt


def fresh_env(env, board, n):
    e = make_env(env, BOARDS[board], batch_size=n, seed=SEED, lane_offset=LANE0, reuse_buffers=True)
    e.call_counter = T0
    return e


def check_sink(env, board, loop, layout):
    n = LOOPS[env][loop]
    ob0, rows, st, acc, cnt = oracle_pass(env, board, n)
    e = fresh_env(env, board, n)
    assert np.array_equal(np_(e.reset()), ob0)
    ctx = (env, board, loop, layout)
    if layout == "returns":
        from gym_pomdp_amd import EpisodeStats
        assert e._discount == 0.95
        stats = e.collect_returns(STEPS, EpisodeStats(e))
        assert last_kernel() == kernel_name(env, layout, loop), (ctx, last_kernel())
        for q, name in enumerate(("ret", "disc", "ret_done", "ret_sum")):
            assert np.array_equal(np_(getattr(stats, name)).view(np.uint64), acc[q].view(np.uint64)), ctx + (name,)
        assert np.array_equal(np_(stats.episodes), cnt[0]) and np.array_equal(np_(stats.steps), cnt[1]), ctx
    else:
        tr = e.collect_synthetic(STEPS) if layout == "columns" else e.collect_synthetic(STEPS, layout=layout)
        assert last_kernel() == kernel_name(env, layout, loop), (ctx, last_kernel())
        cols = tr if layout == "columns" else e.decode_trajectory(tr)
        for k, (a, ob, rew, done) in enumerate(rows):
            assert np.array_equal(np_(cols["action"][k]), a), ctx + (k,)
            assert np.array_equal(np_(cols["ob"][k]), ob), ctx + (k,)
            assert np.array_equal(np_(cols["reward"][k]), rew), ctx + (k,)
            assert np.array_equal(np_(cols["done"][k]), done.astype(bool)), ctx + (k,)
    assert np.array_equal(np_(e.state).view(np.uint32), st), ctx
    assert e.invalid_action_count() == 0


CASES = [(board, loop, layout) for board in BOARDS for loop in LOOPS["rock"] for layout in SINKS[loop]]


@pytest.mark.parametrize("board,loop,layout", CASES, ids=["-".join(c) for c in CASES])
def test_synthetic_rows_of_every_sink_equal_the_oracle(oracle_lib, board, loop, layout):
    check_sink("rock", board, loop, layout)


@pytest.mark.parametrize("loop", list(LOOPS["stochrock"]))
def test_synthetic_rows_of_stochastic_rock_equal_the_oracle(oracle_lib, loop):
    check_sink("stochrock", "7-8", loop, "packed")
    rows = oracle_pass("stochrock", "7-8", LOOPS["stochrock"][loop])[1]
    assert any(((a >= 5) & (ob == 0)).any() for a, ob, _, _ in rows)             # a CHECK the gate refused reads nothing


@pytest.mark.parametrize("loop", list(LOOPS["rock"]))
def test_out_of_range_tape_actions_leave_their_lanes_alone(oracle_lib, loop):
    n = LOOPS["rock"][loop]
    nt = oracle_lib.max_threads()
    o = oracle_lib.OracleEnv("rock")
    rng = np.random.RandomState(1603)
    tape = rng.randint(0, o.n_actions, (STEPS, n)).astype(np.uint8)
    bad_lanes = np.arange(n) % 10 == 3                                           # a tenth of the lanes, in every quad position
    n_bad = int(bad_lanes.sum())
    # every value a byte can hold from n_actions up, 13 (the first one past the table's actions) and 255 among them
    tape[:, bad_lanes] = rng.randint(o.n_actions, 256, (STEPS, n_bad)).astype(np.uint8)
    tape[0, np.flatnonzero(bad_lanes)[:2]] = (o.n_actions, 255)
    e = make_env("rock", {}, batch_size=n, seed=SEED, lane_offset=LANE0)
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, SEED, LANE0, 0, nthreads=nt))
    st0 = st.copy()
    cols = e.decode_trajectory(e.collect_tape(torch.as_tensor(tape, device="cuda"), layout="packed"), STEPS)
    assert last_kernel() == kernel_name("rock", "packed", loop, tape=True), last_kernel()
    done, total = np.zeros(n, np.uint8), 0
    for k in range(STEPS):
        a = tape[k].astype(np.int32)
        ob, rew, done, bad = o.batch_step(st, a, SEED, LANE0, 1 + k, auto_reset=True, done=done, nthreads=nt)
        assert bad == n_bad
        total += bad
        got = [np_(cols[c][k]) for c in ("action", "ob", "reward", "done")]
        assert np.array_equal(got[0], a) and np.array_equal(got[1], ob) and np.array_equal(got[2], rew), (loop, k)
        assert np.array_equal(got[3], done.astype(bool)), (loop, k)
        assert not got[1][bad_lanes].any() and not got[2][bad_lanes].any() and not got[3][bad_lanes].any(), (loop, k)
    state = np_(e.state).view(np.uint32)
    assert np.array_equal(state, st) and np.array_equal(state[:, bad_lanes], st0[:, bad_lanes])
    assert e.invalid_action_count() == total == STEPS * n_bad
