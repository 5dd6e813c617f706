"""BattleShip's fused loops (battleship_steps_quad_kernel and the board builders it calls) at every mask width, on boards that
are edges of the mask arithmetic, with episodes that END inside the launches: under a uniform policy a board larger than 5x5
sees almost no episode end in 64 steps, so the builder pool's refill, its run in the middle of the loop (`again`) and the byte
task lists were only ever reached on 5x5.  The tapes of tests/battleship_tapes.py end episodes on purpose; every comparison is
with the CPU oracle, bit for bit (int rows, all 3 * MW uint32 state words — the next board included —, float64 returns viewed
as uint64), every case asserts the kernel the launcher picked and the coverage counts the oracle's `done` rows give for the
path the case is named for (tests/test_battleship_builder_host.py locates a difference: which builder, which piece).

Boards (MW = mask words, S = ship cells = steps of an episode on a volley tape):
    MW 1   (2, 13) 3, (13, 2) 3   26 cells + 6 = 32 bits exactly; two-wide: every row touches both border columns; S = 5
           (1, 16) 3              col0 == colL, colL = col0 << 0
    MW 2   (8, 6) 4               S = 9
    MW 3   (8, 8) 4, (9, 10) 5, (6, 15) 5     never ran fused before; 90 + 6 = 96 bits exactly; S = 9, 14, 14
    MW 4   (10, 10) 5, (16, 7) 5, (7, 16) 5, (16, 7) 7     16-wide and 16-high; 27 ship cells (S = 27)
Sizes (kernels_common.hip.h; the visited mask is in LDS while lanes * MW <= 2^21, the kernel's name does not show it):
    2^16            a quad per thread, visited mask in LDS, every sink
    2^17            half a quad per thread (", 2") for packed and returns, a quad for columns; visited mask in LDS
    700 416 (MW 3), 2^19 + 4096 (MW 4)      a quad per thread, visited mask in registers (lanes * MW > 2^21)
With MW 1 and 2 the visited mask moves to registers above 2^21 and 2^20 lanes: those forms are left out here.

    a  volley tape, 4 S + 3 steps in launches of 64 (2 S + 3 at the register-mask sizes): every wave queues all 64 * LPT lanes
       at once, and from a launch's second end on the pool runs inside the loop for the whole wave
    b  stagger(S + 3) tape with revisits and out-of-range bytes, 130 steps in launches of 64, begun S - 1 steps after reset():
       lanes end at the first and last step of a launch and on both sides of a launch boundary
    c  one 256-step launch (the default maximum: the pool keeps a lane's deal step in a byte), then 8 steps on the boards built
       after step 255
    d  the returns sink on the tapes of a and b
    e  the synthetic policy from nearly finished states (one ship cell left per lane): a lane ends with probability 1 / cells
       per step, more than a quarter of the batch within 64 steps
    f  the call counter's low word wrapping on a deal step, right after one and on a launch boundary (the builders add the
       deal step to the launch's counter themselves); the hoisted policy block from nearly finished states; the key and lane
       edges K1 and K2 of test_gpu_key_edges
"""
import time

import numpy as np
import pytest
import torch

from battleship_tapes import Tape, coverage, launch_cuts, mask_words, nearly_finished, ship_cells
from test_gpu_parity import make_env, np_
from test_gpu_timed_kernels import fuse64  # noqa: F401  (a fixture: 64 steps per launch)
from test_gpu_key_edges import Ref, coords, last_kernel
from test_gpu_counter_wrap import reset_counter

pytestmark = pytest.mark.gpu

SEED, LANE0, T0 = 0x9E3779B97F4A7C15, 1 << 22, (1 << 33) + 5
N16, N17 = 1 << 16, 1 << 17
B = {"2x13": ((2, 13), 3), "13x2": ((13, 2), 3), "1x16": ((1, 16), 3), "8x6": ((8, 6), 4), "8x8": ((8, 8), 4), "9x10": ((9, 10), 5),
     "6x15": ((6, 15), 5), "10x10": ((10, 10), 5), "16x7": ((16, 7), 5), "7x16": ((7, 16), 5), "16x7-7": ((16, 7), 7)}
WIDE = ("8x8", "9x10", "6x15", "10x10", "16x7", "7x16", "16x7-7")            # MW 3 and MW 4
RETURNS = ("8x8", "9x10", "10x10", "16x7")                                   # d: MW >= 3 returns kernels


def reg_size(board):
    """the smallest full-workgroup batch above 2^19 lanes whose visited mask no longer fits LDS"""
    return {3: 171 * 4096, 4: (1 << 19) + 4096}[mask_words(B[board][0])]


def lpt_of(n, sink):
    return 2 if sink != "columns" and N17 <= n <= 1 << 19 else 4


def kernel_name(board, n, sink, taped):
    mw = mask_words(B[board][0])
    assert (n * mw <= 1 << 21) == (n <= 1 << 19)                              # which side of the visited mask's gate: LDS up to 2^19 here
    return "battleship_steps_quad_kernel<BattleShipEnv<%d>%s%s%s>" % (mw, "" if sink == "columns" else ", " + sink.capitalize(),
                                                                      ", Tape" if taped else "", ", 2" if lpt_of(n, sink) == 2 else "")


def state_of(e):
    return np_(e.state).view(np.uint32)


def fresh_env(r):
    e = make_env("battleship", r.kw, batch_size=r.n, seed=r.seed, lane_offset=r.lane0, reuse_buffers=True)
    e.call_counter = r.t_reset
    assert np.array_equal(np_(e.reset()), r.ob_reset) and np.array_equal(state_of(e), r.st_reset)
    return e


def tape_env(r):
    """a GPU env where the tape's collection begins: reset(), then the prefix (S - 1 steps or a few more), state compared"""
    e = fresh_env(r)
    if r.pre:
        e.collect_tape(torch.as_tensor(r.tape_pre, device="cuda"), layout="packed")
        assert np.array_equal(state_of(e), r.st0)
        e._err.zero_()
    return e


def check_returns(r, e, stats, ctx):
    acc, cnt = r.returns(e._discount, stats.acc.shape[1])
    assert np.array_equal(np_(stats.acc)[:, :r.n].view(np.uint64), acc[:, :r.n].view(np.uint64)), ctx
    assert np.array_equal(np_(stats.cnt)[:, :r.n], cnt[:, :r.n]) and np.array_equal(state_of(e), r.st), ctx
    assert e.invalid_action_count() == r.bad and e.call_counter == r.t0 + 1 + r.steps, ctx


def run_tape(r, board, sink):
    ctx = (board, r.n, sink)
    e = tape_env(r)
    d_tape = torch.as_tensor(r.tape, device="cuda")
    if sink == "returns":
        stats = e.collect_tape(d_tape, layout="returns")
        name = last_kernel()
        check_returns(r, e, stats, ctx)
    else:
        tr = e.collect_tape(d_tape, layout=sink)
        name = last_kernel()
        Ref.check_cols(r, e, e.decode_trajectory(tr, r.steps), ctx, action=sink != "columns")
    assert name == kernel_name(board, r.n, sink, True), (ctx, name)


def report(what, board, n, cov, t_oracle, t_start):
    print("\nBSCOV %s %s n=%d ends=%d again=%d max_pending=%d oracle_s=%.2f total_s=%.2f" % (
        what, board, n, cov["ends"], cov["again"], cov["max_pending"], t_oracle, time.time() - t_start))


# ---- a (+ d): volley ---------------------------------------------------------------------------------------------------------
VOLLEY = [(b, N16, ("packed", "columns") + (("returns",) if b in RETURNS else ()), 4) for b in B] + \
         [(b, N17, ("packed",) + (("returns",) if b in RETURNS else ()), 4) for b in WIDE] + \
         [(b, reg_size(b), ("packed",), 2) for b in WIDE]


@pytest.mark.parametrize("board,n,sinks,episodes", VOLLEY, ids=["%s-%d" % c[:2] for c in VOLLEY])
def test_volley_tapes_equal_the_oracle(oracle_lib, fuse64, board, n, sinks, episodes):
    start = time.time()
    size, max_len = B[board]
    S = ship_cells(max_len)
    steps = episodes * S + 3
    r = Tape(oracle_lib, size, max_len, n, steps, SEED, LANE0, T0)
    t_oracle = time.time() - start
    ends_per_launch = [len([s for s in range(lo, lo + k) if s % S == S - 1]) for lo, k in zip(range(0, steps, 64), launch_cuts(steps, 64))]
    for lpt in sorted({lpt_of(n, s) for s in sinks}):
        cov = r.coverage(64, lpt)
        assert cov["ends"] == n * episodes and (r.done.sum(axis=0) == episodes).all(), (board, n)
        assert cov["again"] == n * sum(k >= 2 for k in ends_per_launch) > 0, (board, n, cov)
        assert cov["max_pending"] == 64 * lpt, (board, n, cov)
    for sink in sinks:
        run_tape(r, board, sink)
    report("volley", board, n, cov, t_oracle, start)


# ---- b (+ d): stagger, revisits, out-of-range bytes ------------------------------------------------------------------------------
STAGGER = [("2x13", N16, ("packed",)), ("8x8", N16, ("packed", "returns")), ("9x10", N16, ("packed", "returns")),
           ("16x7-7", N16, ("packed",)), ("10x10", N16, ("returns",)), ("16x7", N16, ("returns",)),
           ("8x8", N17, ("packed", "returns")), ("9x10", N17, ("returns",)), ("10x10", N17, ("returns",)), ("16x7", N17, ("returns",))]


@pytest.mark.parametrize("board,n,sinks", STAGGER, ids=["%s-%d" % c[:2] for c in STAGGER])
def test_staggered_tapes_equal_the_oracle(oracle_lib, fuse64, board, n, sinks):
    start = time.time()
    size, max_len = B[board]
    S = ship_cells(max_len)
    r = Tape(oracle_lib, size, max_len, n, 130, SEED, LANE0, T0, schedule="stagger", period=S + 3, revisit=True, bad=True, pre=S - 1)
    t_oracle = time.time() - start
    for s in (0, 63, 64, 127, 128):
        assert r.done[s].any(), (board, n, s)                                # a launch's first and last step, both sides of a boundary
    assert r.bad == int((r.tape >= size[0] * size[1]).sum()) > 0 and (r.reward == -10).any(), (board, n)
    cov = r.coverage(64, lpt_of(n, sinks[0]))
    assert cov["ends"] > n and cov["again"] > 0, (board, n, cov)
    for sink in sinks:
        run_tape(r, board, sink)
    report("stagger", board, n, cov, t_oracle, start)


# ---- c: the longest launch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("board", ["8x8", "10x10"])
def test_a_256_step_launch_deals_at_its_first_and_last_step(oracle_lib, board):
    from gym_pomdp_amd import _native
    assert _native.FUSE_MAX_DEFAULT == 256
    start = time.time()
    size, max_len = B[board]
    S, n = ship_cells(max_len), N16
    # lane class m (= i mod P) ends at steps j (S + m) - 1 after reset(): the shortest prefix after which some class ends at
    # step 0 and some class at step 255 of the collection (8x8: 8 steps, 264 = 12 * 22; 10x10: 14, 15 | 270)
    pre = min(p for p in range(S - 1, 4 * S) if all(any((p + 1 + s) % L == 0 for L in range(S, 2 * S + 3)) for s in (0, 255)))
    r = Tape(oracle_lib, size, max_len, n, 256 + 8, SEED, LANE0, T0, schedule="stagger", period=S + 3, pre=pre)
    t_oracle = time.time() - start
    assert r.done[0].any() and r.done[255].any(), board                      # boards dealt at deal steps 0 and 255 of the launch
    cov = coverage(r.done.astype(bool), [256, 8], 4)
    assert cov["again"] == n and (r.done[:256].sum(axis=0) >= 2).all(), (board, cov)   # every lane ends twice or more in the long launch
    e = tape_env(r)
    lo = 0
    for k in (256, 8):                                                       # the second collection plays on the boards built after step 255
        tr = e.collect_tape(torch.as_tensor(r.tape[lo:lo + k], device="cuda"), layout="packed")
        assert last_kernel() == kernel_name(board, n, "packed", True), (board, k, last_kernel())
        cols = e.decode_trajectory(tr, k)
        ctx = (board, lo, k)
        assert np.array_equal(np_(cols["action"]).astype(np.int32), r.action[lo:lo + k]), ctx
        assert np.array_equal(np_(cols["ob"]).astype(np.int32), r.ob[lo:lo + k]), ctx
        assert np.array_equal(np_(cols["reward"]).astype(r.reward.dtype), r.reward[lo:lo + k]), ctx
        assert np.array_equal(np_(cols["done"]), r.done[lo:lo + k].astype(bool)), ctx
        lo += k
    assert r.done[256:].any(), board
    assert np.array_equal(state_of(e), r.st) and e.invalid_action_count() == 0 and e.call_counter == r.t0 + 1 + r.steps, board
    report("launch256", board, n, cov, t_oracle, start)


# ---- e, f: the synthetic policy from nearly finished states --------------------------------------------------------------------
class Synth(object):
    """The oracle under the synthetic policy from nearly finished states (battleship_tapes.nearly_finished of the state after
    reset() at t0); attributes as Ref has them."""

    def __init__(self, ol, board, n, steps, seed, lane0, t0):
        size, max_len = B[board]
        self.kw = dict(board_size=size, max_len=max_len)
        self.ol, self.o, self.n, self.steps = ol, ol.OracleEnv("battleship", **self.kw), n, steps
        self.seed, self.lane0, self.t0, self.t_reset, self.tape = seed, lane0, t0, t0, None
        o, nt = self.o, ol.max_threads()
        self.nt = nt
        st = o.new_state(n)
        self.ob_reset = o.batch_reset(st, seed, lane0, t0, nthreads=nt)
        self.st_reset = st.copy()
        st, _ = nearly_finished(st, size)
        self.st0 = st.copy()
        done = np.zeros(n, np.uint8)
        rows, self.bad = [], 0
        for k in range(steps):
            t = t0 + 1 + k
            a = ol.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt)
            ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
            self.bad += bad
            rows.append((a, ob, rew, done.copy()))
        self.st = st
        self.action, self.ob, self.reward, self.done = (np.stack([r[i] for r in rows]) for i in range(4))
        self.a_next = ol.synthetic_actions(n, seed, lane0, t0 + 1 + steps, o.n_actions, nthreads=nt)

    returns = Ref.returns

    def env(self):
        e = fresh_env(self)
        e.set_state(torch.as_tensor(self.st0.view(np.int32), device="cuda"))
        assert np.array_equal(state_of(e), self.st0) and e.call_counter == self.t0 + 1
        return e


def run_synth(r, board, sink):
    ctx = (board, r.n, sink, r.t0)
    e = r.env()
    if sink == "returns":
        stats = e.collect_returns(r.steps)
        name = last_kernel()
        check_returns(r, e, stats, ctx)
    else:
        tr = e.collect_synthetic(r.steps, layout=sink)
        name = last_kernel()
        Ref.check_cols(r, e, e.decode_trajectory(tr), ctx)
        if sink == "columns":
            assert np.array_equal(np_(tr["action"][r.steps]), r.a_next), ctx
    assert name == kernel_name(board, r.n, sink, False), (ctx, name)


NEARLY = [(b, N16, ("packed", "returns")) for b in RETURNS] + [("8x8", N17, ("packed",)), ("10x10", N17, ("packed",))]


@pytest.mark.parametrize("board,n,sinks", NEARLY, ids=["%s-%d" % c[:2] for c in NEARLY])
def test_synthetic_policy_from_nearly_finished_states(oracle_lib, fuse64, board, n, sinks):
    start = time.time()
    r = Synth(oracle_lib, board, n, 64, SEED, LANE0, T0)
    t_oracle = time.time() - start
    assert r.done.any(axis=0).mean() >= .25, (board, n)                      # 1 - (1 - 1 / cells)^64 > .4 on every board here
    cov = coverage(r.done.astype(bool), [64], lpt_of(n, sinks[0]))
    for sink in sinks:
        run_synth(r, board, sink)
    report("nearly", board, n, cov, t_oracle, start)


@pytest.mark.parametrize("w", [8, 9, 17, 18, 63, 64])
def test_the_counter_wraps_around_a_deal_step(oracle_lib, fuse64, w):
    """volley on (8, 8): boards are dealt at steps 8, 17, 26, ..; the env counter's low word becomes 0 at step w — on a deal
    step, right after one, on the launch's last step and (w = 64, 80 steps) on the second launch's first"""
    start = time.time()
    size, max_len = B["8x8"]
    steps = 80 if w == 64 else 64
    t0 = reset_counter(w)
    assert (t0 + 1 + w) % (1 << 32) == 0 and (t0 + 1) >> 32 == ((t0 + 1 + w) >> 32) - 1
    r = Tape(oracle_lib, size, max_len, N16, steps, SEED, LANE0, t0)
    t_oracle = time.time() - start
    assert r.done[8].all() and r.done[17].all() and r.done.sum() == N16 * (steps // 9)
    cov = r.coverage(64, 4)
    assert cov["again"] == N16 and cov["max_pending"] == 256, cov           # (w = 64: the second launch, 16 steps, holds one end)
    run_tape(r, "8x8", "packed")
    report("wrap-w%d" % w, "8x8", N16, cov, t_oracle, start)


@pytest.mark.parametrize("w", [0, 1, 40])
def test_the_hoisted_policy_block_across_the_wrap_from_nearly_finished_states(oracle_lib, fuse64, w):
    start = time.time()
    t0 = reset_counter(w)
    r = Synth(oracle_lib, "8x8", N16, 64, SEED, LANE0, t0)
    t_oracle = time.time() - start
    assert r.done[:max(w, 1)].any() and r.done[w:].any() and r.done.any(axis=0).mean() >= .25, w
    cov = coverage(r.done.astype(bool), [64], 4)
    run_synth(r, "8x8", "packed")
    report("hoist-w%d" % w, "8x8", N16, cov, t_oracle, start)


@pytest.mark.parametrize("K", ["K1", "K2"])
def test_volley_at_the_key_and_lane_edges(oracle_lib, fuse64, K):
    """K1: the batch's last quad is the top one of the lane range (wave0 + bidx up to 2^32 - 1) and the counter carries into its
    high word inside the launch; K2: k0 = 0, k1 = 1 in the builders' Philox call, t_hi carries to 0xFFFFFFFF"""
    start = time.time()
    size, max_len = B["8x8"]
    seed, lane0, t0 = coords(K, N16)
    assert K != "K1" or lane0 + N16 == 1 << 32
    r = Tape(oracle_lib, size, max_len, N16, 4 * 9 + 3, seed, lane0, t0)
    t_oracle = time.time() - start
    cov = r.coverage(64, 4)
    assert cov["ends"] == 4 * N16 and cov["again"] == N16 and cov["max_pending"] == 256, cov
    run_tape(r, "8x8", "packed")
    report("volley-" + K, "8x8", N16, cov, t_oracle, start)
