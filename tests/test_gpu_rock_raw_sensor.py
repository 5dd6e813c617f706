"""RockSample's quad and half-quad loops (steps_quad_kernel / steps_quad_popc_kernel) since the lane step compares the raw
sensor word and the reset-tie filter of boards with at most eight rocks is numeric: whole batches against the oracle.

Each case is a 16-step tape — the launcher's minimum for the table loops — on the smallest batch the launcher gives the loop
(3 << 18 lanes: a quad per thread; (3 << 17) + 4096: half a quad), every lane's 16 records and its final state:
  * both reset-tie filters: RockSample(7,8) takes the numeric one, RockSample(11,11) the popcount one; the tapes are uniform
    actions, so every step some lanes leave the board and start a fresh episode from their sensor word;
  * the sensor at distance 0, whose table entry is saturated (always right): a few tape moves put every lane on a rock's
    cell, then a second tape's rows CHECK the rock under the agent;
  * StochasticRock through the quad loop (the gate block besides the sensor block), at its own smallest batch, 1 << 19."""
import numpy as np
import pytest
import torch

from test_gpu_parity import make_env, np_

pytestmark = pytest.mark.gpu

STEPS = 16
LOOPS = {"quad": (3 << 18, ""), "half": ((3 << 17) + 4096, ", 2")}
SEED, LANE0 = 20251, 1 << 22


def kernel_name(env, loop):
    return "steps_quad_kernel<%s<1>, Packed, Tape%s>" % ("StochasticRockEnv" if env == "stochrock" else "RockEnv", LOOPS[loop][1])


def run_tapes(oracle_lib, env, kw, loop, tapes):
    """reset, then one collect_tape per tape: every row of every launch against oracle.batch_step, then the state"""
    from gym_pomdp_amd import _native
    n = tapes[0].shape[1]
    nt = oracle_lib.max_threads()
    e = make_env(env, kw, batch_size=n, seed=SEED, lane_offset=LANE0)
    o = oracle_lib.OracleEnv(env, **kw)
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, SEED, LANE0, 0, nthreads=nt))
    done, t, rows = np.zeros(n, np.uint8), 1, []
    for tape in tapes:
        assert tape.shape == (STEPS, n) and int(tape.max()) < o.n_actions
        cols = e.decode_trajectory(e.collect_tape(torch.as_tensor(tape, device="cuda"), layout="packed"), STEPS)
        assert _native.lib().pomdp_last_fused_kernel().decode() == kernel_name(env, loop), _native.lib().pomdp_last_fused_kernel()
        for k in range(STEPS):
            a = tape[k].astype(np.int32)
            ob, rew, done, bad = o.batch_step(st, a, SEED, LANE0, t, auto_reset=True, done=done, nthreads=nt)
            t += 1
            ctx = (env, kw, loop, t)
            assert bad == 0
            assert np.array_equal(np_(cols["action"][k]), a), ctx
            assert np.array_equal(np_(cols["ob"][k]), ob), ctx
            assert np.array_equal(np_(cols["reward"][k]), rew), ctx
            assert np.array_equal(np_(cols["done"][k]), done.astype(bool)), ctx
            rows.append((a, ob, done.copy()))
        assert np.array_equal(np_(e.state).view(np.uint32), st), (env, kw, loop)
    assert e.invalid_action_count() == 0
    return rows


@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("board", ["7-8", "11-11"])
def test_both_reset_filters_against_the_oracle(oracle_lib, board, loop):
    kw = {} if board == "7-8" else dict(board_size=11, num_rocks=11)
    n, n_actions = LOOPS[loop][0], 5 + (8 if board == "7-8" else 11)
    tape = np.random.RandomState(len(board) + n % 977).randint(0, n_actions, (STEPS, n)).astype(np.uint8)
    rows = run_tapes(oracle_lib, "rock", kw, loop, [tape])
    assert all(d.any() for _, _, d in rows) and sum(int(d.sum()) for _, _, d in rows) > n // 4   # fresh episodes in every row
    assert any(((a > 4) & (ob == 1)).any() for a, ob, _ in rows) and any(((a > 4) & (ob == 2)).any() for a, ob, _ in rows)


@pytest.mark.parametrize("loop", list(LOOPS))
def test_sensor_at_distance_zero(oracle_lib, loop):
    """RockSample(7,8) starts at (0, 3); rock 1 lies at (0, 1), two steps SOUTH, and rock 4 at (2, 4), EAST, EAST, NORTH.  Even
    lanes walk to the one, odd lanes to the other (CHECKs of rock 0 fill the first tape); the second tape's row 0, and every
    row after it, CHECKs the rock under the agent: the saturated entry, where the reading IS the rock's value."""
    from gym_pomdp_amd import tables
    n = LOOPS[loop][0]
    rocks = tables.ROCK_CONFIG[7][2]
    assert tuple(rocks[1]) == (0, 1) and tuple(rocks[4]) == (2, 4) and int(tables.ROCK_THR[0]) >> 26 == 1 << 27
    walk = np.full((STEPS, n), 5, np.uint8)
    walk[0:2, 0::2] = 2                                                     # SOUTH, SOUTH
    walk[0:2, 1::2] = 1                                                     # EAST, EAST,
    walk[2, 1::2] = 0                                                       # NORTH
    check = np.empty((STEPS, n), np.uint8)
    check[:, 0::2] = 5 + 1
    check[:, 1::2] = 5 + 4
    rows = run_tapes(oracle_lib, "rock", {}, loop, [walk, check])
    assert not any(d.any() for _, _, d in rows)                             # nobody left the board: every lane stands on its rock
    for a, ob, _ in rows[STEPS:]:
        assert np.isin(ob, (1, 2)).all() and (ob == 1).any() and (ob == 2).any()
        assert np.array_equal(ob, rows[STEPS][1])                           # always right: the same reading sixteen times


def test_stochastic_rock_through_the_quad_loop(oracle_lib):
    n = 1 << 19                                                             # QUAD_MIN_STOCHROCK (kernels_common.hip.h)
    tape = np.random.RandomState(7).randint(0, 13, (STEPS, n)).astype(np.uint8)
    rows = run_tapes(oracle_lib, "stochrock", {}, "quad", [tape])
    assert any(((a > 4) & (ob == 0)).any() for a, ob, _ in rows)           # a CHECK the gate refused reads nothing
