"""The quad-per-thread step loops where a call counter's low word wraps inside a launch.  Their quad-shared Philox blocks take
round 3's product of word 0 from in front of the loop (philox.hip.h: philox_hoist) — valid for one high word of the counter —
and the loop runs as stretches that end where a counter's low word becomes 0.  tests/test_philox_hoist_host.py shows that a
product carried across that step gives other words; here the env's counter wraps at a chosen step w of a 64-step launch (the
policy's counter, one ahead, at step w - 1) and every row is compared with the CPU oracle, bit for bit.

    w = 0       the launch's first step draws the env's block under the new high word; the policy's first actions (first())
                and its block of step 0 straddle the wrap the other way round at w = 1
    w = 1       the policy's counter of step 0 has low word 0: first() draws under the OLD high word
    w = 10, 11 / 40, 41 / 54, 55 / 61, 62     an even and an odd step inside each of the four priority segments of a 64-step
                launch (LoopPrio: they end at steps 36, 52, 60, 64); the tape loop, unrolled by two, keeps a product per parity
    w = 63      the last step
    w = 64      of an 80-step collection cut into launches of 64 and 16: the env's wrap is the second launch's first step, the
                policy's the first launch's last

Sizes are the launcher's gates (test_launcher_picks_the_documented_kernel_per_shard_size); the kernel is asserted in every case."""
import numpy as np
import pytest
import torch

from test_gpu_parity import np_
from test_gpu_timed_kernels import _tape, fuse64  # noqa: F401  (fuse64: a fixture — 64 steps per launch)
from test_gpu_key_edges import Ref, last_kernel

pytestmark = pytest.mark.gpu

SEED, LANE0 = 0x9E3779B97F4A7C15, 1 << 22
WRAPS = (0, 1, 10, 11, 40, 41, 54, 55, 61, 62, 63, 64)
# (id, env, kwargs, n, kernel family, sinks walked on the one oracle pass)
LOOPS = [
    ("rock", "rock", {}, 3 << 18, "steps_quad_kernel<RockEnv<1>", ("Packed", "Returns")),
    ("rock-tape", "rock", {}, 3 << 18, "steps_quad_kernel<RockEnv<1>", ("Tape",)),
    ("rock11-popc", "rock", dict(board_size=11, num_rocks=11), 3 << 18, "steps_quad_kernel<RockEnv<1>", ("Packed",)),
    ("rock15", "rock", dict(board_size=15, num_rocks=15), 3 << 18, "steps_quad_kernel<RockEnv<2>", ("Packed",)),
    ("stochrock", "stochrock", {}, 1 << 19, "steps_quad_kernel<StochasticRockEnv<1>", ("Packed",)),       # gate_fx as well as sensor_fx
    ("tiger", "tiger", {}, 1 << 19, "steps_quad_generic_kernel<TigerEnv", ("Packed",)),                   # SyntheticQuad alone
]
CASES = [(c, w) for c in LOOPS for w in WRAPS]


def reset_counter(w):
    """the call counter reset() runs at, such that step w of the collection (counter t0 + 1 + w) is the first with a low word of
    0; the high word goes 0 -> 1 at even w and 0xFFFFFFFE -> 0xFFFFFFFF at odd w"""
    hi = 1 if w % 2 == 0 else 0xFFFFFFFF
    return (hi << 32) - 1 - w


@pytest.mark.parametrize("case,w", CASES, ids=["%s-w%d" % (c[0], w) for c, w in CASES])
def test_rows_equal_the_oracle_across_the_wrap(oracle_lib, fuse64, case, w):
    _, env, kw, n, family, sinks = case
    steps = 80 if w == 64 else 64
    t0 = reset_counter(w)
    assert (t0 + 1 + w) % (1 << 32) == 0 and (t0 + 1) >> 32 == ((t0 + 1 + w) >> 32) - (w > 0)
    tape = d_tape = None
    if "Tape" in sinks:
        tape = _tape(np.random.RandomState(w), oracle_lib.OracleEnv(env, **kw).n_actions, steps, n, 4096)
        d_tape = torch.as_tensor(tape, device="cuda")
    r = Ref(oracle_lib, env, kw, n, steps, SEED, LANE0, t0, tape=tape)
    for sink in sinks:
        ctx = (env, kw, n, w, sink)
        e = r.env(env, kw)
        if sink == "Returns":
            stats = e.collect_returns(steps)
            name = last_kernel()
            acc, cnt = r.returns(e._discount, stats.acc.shape[1])
            assert np.array_equal(np_(stats.acc)[:, :n].view(np.uint64), acc[:, :n].view(np.uint64)), ctx
            assert np.array_equal(np_(stats.cnt)[:, :n], cnt[:, :n]) and np.array_equal(np_(e.state).view(np.uint32), r.st), ctx
        else:
            tr = e.collect_synthetic(steps, layout="packed") if tape is None else e.collect_tape(d_tape, layout="packed")
            name = last_kernel()
            r.check_cols(e, e.decode_trajectory(tr) if tape is None else e.decode_trajectory(tr, steps), ctx)
        assert name == family + {"Packed": ", Packed>", "Returns": ", Returns>", "Tape": ", Packed, Tape>"}[sink], (ctx, name)
    assert r.done.any(), (env, w)                                       # episodes ended and restarted inside the launch
