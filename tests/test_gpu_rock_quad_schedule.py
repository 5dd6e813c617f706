"""RockSample's quad and half-quad loops (steps_quad_kernel / steps_quad_popc_kernel, csrc/fused_impl.hip.h) under the synthetic
policy, since the policy's Philox block is issued under the lane step's table reads: every row, the returns statistics and the
state a launch leaves, against the CPU oracle, at the smallest batches that take these loops —

    quad   3 * 2^18 lanes (QUAD_MIN_ROCK; StochasticRock: 2^19, QUAD_MIN_STOCHROCK), packed records and the returns sink;
    half   ROCK_PAIR_MIN_LANES = 3 * 2^17 + 1 rounded up to whole 1024-lane workgroups, packed records (the returns sink has no
           half-quad form): the policy's block is the pair's, computed at even steps only.

Launch lengths 16, 17 and 33: the launcher's shortest table-driven launch, odd and even lengths (the half-quad form ends on
either parity of its shared block), and with 17 and 33 a step past a boundary of the loop's priority segments.  Boards (7,8),
(4,3) and (2,1) take the 16-byte table form (RecWide), (11,11) the 8-byte one (RecRot, steps_quad_popc_kernel — under the same
reported name).  One packed launch starts nine steps below a multiple of 2^32 of the call counter: the stretch of hoisted Philox
products ends in mid-launch (the policy's one step before the env's), with table reads in flight."""
import numpy as np
import pytest

from test_gpu_parity import np_
from test_gpu_key_edges import Ref, last_kernel

pytestmark = pytest.mark.gpu

SEED, LANE0, T0 = 20261020, 1 << 20, (1 << 32) + 3
QUAD, HALF, STOCH = 3 << 18, (3 << 17) + 1024, 1 << 19
BOARDS = {"7-8": {}, "4-3": dict(board_size=4, num_rocks=3), "2-1": dict(board_size=2, num_rocks=1), "11-11": dict(board_size=11, num_rocks=11)}
KS = (16, 17, 33)
CASES = [("rock", b, QUAD, k, "") for b in BOARDS for k in KS] + [("rock", b, HALF, k, ", 2") for b in ("7-8", "11-11") for k in KS]
CASES.append(("stochrock", "7-8", STOCH, 17, ""))
NAMES = {"rock": "RockEnv<1>", "stochrock": "StochasticRockEnv<1>"}


def run_case(oracle_lib, env, board, n, k, half, t0):
    kw = BOARDS[board]
    r = Ref(oracle_lib, env, kw, n, k, SEED, LANE0, t0)
    assert r.done.any() and not r.done.all()                                    # auto-resets happen, and not everywhere
    e = r.env(env, kw)
    tr = e.collect_synthetic(k, layout="packed")
    assert last_kernel() == "steps_quad_kernel<%s, Packed%s>" % (NAMES[env], half), last_kernel()
    r.check_cols(e, e.decode_trajectory(tr, k), (env, board, n, k, "packed"))
    if half:
        return
    e = r.env(env, kw)
    stats = e.collect_returns(k)
    assert last_kernel() == "steps_quad_kernel<%s, Returns>" % NAMES[env], last_kernel()
    acc, cnt = r.returns(e._discount, stats.acc.shape[1])
    assert np.array_equal(np_(stats.acc)[:, :n].view(np.uint64), acc[:, :n].view(np.uint64)), (env, board, n, k)
    assert np.array_equal(np_(stats.cnt)[:, :n], cnt[:, :n]) and np.array_equal(np_(e.state).view(np.uint32), r.st), (env, board, n, k)


@pytest.mark.parametrize("env,board,n,k,half", CASES, ids=["%s-%s-%d-%d" % c[:4] for c in CASES])
def test_rows_returns_and_state_equal_the_oracle(oracle_lib, env, board, n, k, half):
    run_case(oracle_lib, env, board, n, k, half, T0)


def test_call_counter_crosses_a_multiple_of_2_32_inside_the_launch(oracle_lib):
    """17 steps from call counter 2^32 - 9: the env's counter carries into its high word at the ninth step, the policy's at the
    eighth — both stretches end inside the launch."""
    t0, k = (1 << 32) - 9, 17
    assert t0 + 1 < 1 << 32 < t0 + k
    run_case(oracle_lib, "rock", "7-8", QUAD, k, "", t0)
