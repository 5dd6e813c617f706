"""The 2^-27 paths of RockSample's quad-per-thread and half-quad-per-thread fused loops (steps_quad_kernel).

Those loops read the table entries of all of a thread's lanes first and take ONE branch for the lanes whose sensor draw the
high word leaves undecided, and one for the lanes whose fresh episode has a rock on the 2^52 boundary; the tie fixtures
(tests/golden/ties_rock.npz, ties_rock_auto.npz: the reference's own outcomes on lanes found by tests/golden/find_ties.py)
otherwise only reach the kernels of env.step().  Here each tied lane sits in a batch of the smallest size the launcher gives
the loop, and a 16-step tape — the launcher's minimum for the table loops — holds the fixture's action for that lane in row 0
and CHECK rock 0, which changes no state, everywhere else."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_parity import make_env, np_

pytestmark = pytest.mark.gpu

STEPS = 16
LOOPS = {"quad": (3 << 18, "steps_quad_kernel<RockEnv<1>, Packed, Tape>"),
         "half": ((3 << 17) + 4096, "steps_quad_kernel<RockEnv<1>, Packed, Tape, 2>")}


def run_tied_lane(n, kernel, seed, lane, action, state0):
    """-> (row 0's (ob, reward, done) of the tied lane, its decoded state after the launch)"""
    from gym_pomdp_amd import _native
    L = _native.lib()
    base = max(0, (lane & ~3) - n // 2)
    col = lane - base
    e = make_env("rock", {}, batch_size=n, seed=seed, lane_offset=base)
    e.reset()
    assert np.array_equal(np_(e.decode_state()[col]), state0), (lane, n)
    tape = np.full((STEPS, n), 5, np.uint8)
    tape[0, col] = action
    cols = e.decode_trajectory(e.collect_tape(torch.as_tensor(tape, device="cuda"), layout="packed"), STEPS)
    assert L.pomdp_last_fused_kernel().decode() == kernel, L.pomdp_last_fused_kernel()
    assert e.invalid_action_count() == 0
    assert int(cols["action"][0][col]) == action
    return (int(cols["ob"][0][col]), int(cols["reward"][0][col]), int(cols["done"][0][col])), np_(e.decode_state()[col])


@pytest.mark.parametrize("loop", list(LOOPS))
def test_sensor_tie_in_the_quad_loops(loop):
    """Every step case of ties_rock.npz (a CHECK whose draw's high word equals the threshold's): row 0's record of the tied
    lane decodes to the reference's (ob, reward, done)."""
    n, kernel = LOOPS[loop]
    g = dict(np.load(os.path.join(GOLDEN, "ties_rock.npz")))
    seed, n_reset = int(g["seed"]), int(g["n_reset"])
    assert len(g["lanes"]) > n_reset
    for i in range(n_reset, len(g["lanes"])):
        lane = int(g["lanes"][i])
        got, _ = run_tied_lane(n, kernel, seed, lane, int(g["actions"][i]), g["state0"][i])
        assert got == (int(g["ob"][i]), int(g["reward"][i]), int(g["done"][i])), (loop, lane)


@pytest.mark.parametrize("loop", list(LOOPS))
def test_reset_tie_in_the_quad_loops(loop):
    """Every lane of ties_rock_auto.npz (a done step whose fresh episode has a rock decided by the LOW word): row 0 is the
    reference's record with done = 1, and the state the launch leaves — fifteen CHECKs later — is the episode the reference dealt."""
    n, kernel = LOOPS[loop]
    g = dict(np.load(os.path.join(GOLDEN, "ties_rock_auto.npz")))
    seed = int(g["seed"])
    for i, lane in enumerate(g["lanes"]):
        lane = int(lane)
        got, state = run_tied_lane(n, kernel, seed, lane, int(g["actions"][i]), g["state0"][i])
        assert got == (int(g["ob"][i]), int(g["reward"][i]), 1), (loop, lane)
        assert np.array_equal(state, g["state"][i]), (loop, lane)
