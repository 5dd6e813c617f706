"""Every launch form under the constructor parameters that, until this module, only step() met: StochasticRockEnv(p_move),
TagEnv(move_prob, num_opponents, obs_cells) and NetworkEnv(n_machines, problem_type).  The kernels keep hand-specialised copies
of the same parameter-dependent line (the action gate's sense flag act_gt, Tag's flee_word, Network's machines mask and byte
tables); here each copy runs against the CPU oracle, which tests/test_reference_live.py pins to the reference at these
configurations.  Every comparison is bit for bit: int rows, uint32 state words, float32 rewards as stored, float64 returns
viewed as uint64.

Sizes are the launcher's gates (kernels_common.hip.h), the smallest batches at which each loop is still picked; every fused
launch is checked against the kernel name the launcher documents.  All launches run at seed 0x9E3779B97F4A7C15 (both key words
set), lane_offset 2^22 and a call counter above 2^33 (tests/test_env_params_host.py), but the particle filter's (its helper's
own seed) and the tie cases' (the seeds found there).

Surfaces: s1 step(); s2 collect_synthetic columns at the quad gate; s3 the same at 2^15 lanes (one lane per thread), 24 and 8
steps; s4 the packed sink at 3 * 2^17 (half a quad per thread); s5 collect_tape(packed) at 2^19 and 4099; s6 collect_returns,
24 steps then 5 more; s7 finish_episodes with frozen lanes; s8 run_controller; s9 rollout / plan / plan_step; s10 the fused
heuristic loop; s11 the particle update.  Coverage is asserted from the ORACLE's rows and pre-states, never from the kernels'.

Network: network_steps_quad_kernel<1, L, false> (up to 8 machines without the state table) cannot be reached: the state-table
form takes every configuration of at most 10 machines whose thresholds' top 16 bits are non-zero, and the thresholds are
fixed."""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controller_restatement as cr  # noqa: E402
import test_gpu_controller as tgc  # noqa: E402
from test_env_params_host import LANE0, SEED, T0, TIE_LANES, TIE_SEED, tie_lanes  # noqa: E402
from test_gpu_episodes import Pair, check_returns, check_rows, random_tape  # noqa: E402
from test_gpu_key_edges import Ref, kwid, last_kernel  # noqa: E402
from test_gpu_parity import make_env, np_  # noqa: E402
from test_gpu_particles import run_filter  # noqa: E402
from test_gpu_timed_kernels import _heuristic_fused_vs_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

GATE = 1 << 19                       # QUAD_MIN_STOCHROCK = QUAD_MIN_TAG = QUAD_MIN_NETWORK = STEP_QUAD_MIN_LANES
SMALL = 1 << 15                      # one lane per thread, full workgroups
PAIR = 3 << 17                       # STOCHROCK_PAIR_MIN_LANES = TAG_PAIR_MIN_LANES: half a quad per thread
RAGGED = 4099

ROCK = [dict(p_move=.4), dict(p_move=.95)]                  # gt / le
ROCK_HALF = dict(p_move=.5)
ROCK15 = dict(board_size=15, num_rocks=15, p_move=.4)        # two state words
TAG = [dict(move_prob=.3), dict(move_prob=.55)]             # gt / le, one opponent
TAG_HALF = dict(move_prob=.5)
TAG_MULTI = [dict(num_opponents=2, move_prob=.3), dict(num_opponents=4, move_prob=.4)]
TAG63, TAG64 = dict(obs_cells=63), dict(obs_cells=64)       # tab_ok's obs_cells < 64, from both sides
RING, LEGS = 2, 3
NET = [dict(n_machines=M, problem_type=T) for M, T in ((1, RING), (2, RING), (3, RING), (4, LEGS), (8, RING), (9, RING), (10, RING),
                                                       (11, RING), (17, RING), (24, RING), (25, LEGS), (32, RING))]
NET4 = [NET[0], NET[3], NET[8], NET[11]]                     # (1, ring), (4, 3legs), (17, ring), (32, ring)


def ids(cases):
    return ["%s%s" % (c[0], kwid(c[1])) for c in cases]


def env_name(env, kw):
    return {"stochrock": "StochasticRockEnv<%d>" % (2 if kw.get("num_rocks", 8) > 12 else 1), "tag": "TagEnv", "network": "NetworkEnv"}[env]


def fused_name(env, kw, n, k, sink="Columns", taped=False):
    """the kernel the launcher documents for a fused launch of k steps over n lanes (fused_impl.hip.h, launch_steps_fused_l),
    at the sizes this module uses"""
    cols = sink == "Columns"
    lname = ("" if cols else ", " + sink) + (", Tape" if taped else "")
    full = n % 1024 == 0
    if env == "network" and full and n >= GATE:
        M = kw["n_machines"]
        return "network_steps_quad_kernel<%d, %s, %s%s>" % (2 if M <= 10 else (M + 7) // 8, sink, "true" if M <= 10 else "false",
                                                            ", Tape" if taped else "")
    if env == "tag" and full and kw.get("num_opponents", 1) == 1:
        tab = k >= 16 and kw.get("obs_cells", 29) < 64
        if sink in ("Packed", "Narrow", "Returns") and PAIR <= n < 3 << 18 and tab:
            return "tag_steps_quad_kernel<true%s, 2>" % lname
        if n >= GATE:
            return "tag_steps_quad_kernel<%s%s>" % ("true" if tab else "false", lname)
    if env == "stochrock" and full and k >= 16:
        if sink in ("Packed", "Narrow") and PAIR <= n < GATE:
            return "steps_quad_kernel<%s%s, 2>" % (env_name(env, kw), lname)
        if n >= GATE:
            return "steps_quad_kernel<%s%s>" % (env_name(env, kw), lname)
    if taped:                                                # the general loop on a tape (this module: ragged batches only)
        assert n % 256
        return "steps_kernel<%s, 1, false%s%s>" % (env_name(env, kw), "" if cols else ", false", lname)
    if env == "tag" and n >= GATE:
        return "steps_kernel<TagEnv, 2, %s%s%s>" % ("true" if n % 512 == 0 else "false", "" if cols else ", false", lname)
    return "steps_kernel<%s, 1, %s%s%s>" % (env_name(env, kw), "true" if n % 256 == 0 else "false", "" if cols else ", false", lname)


def paramcov(env, kw, surface, n, cov, oracle_s, t_start):
    print("PARAMCOV %s %s %s n=%d %s oracle_s=%.2f total_s=%.2f" % (env, kwid(kw), surface, n, cov, oracle_s, time.time() - t_start))


class Traj(Ref):
    """test_gpu_key_edges.Ref at this module's coordinates, optionally from a state the caller sets (`start`: uint32 [words, n],
    handed to set_state() after reset()), keeping the oracle's state before and after the steps in `keep` for the coverage
    assertions.  Computed once per case and compared with every sink of the case."""

    def __init__(self, ol, env, kw, n, steps, seed=SEED, lane0=LANE0, t0=T0, tape=None, start=None, keep=()):
        t_or = time.time()
        self.ol, self.o, self.n, self.steps = ol, ol.OracleEnv(env, **kw), n, steps
        self.seed, self.lane0, self.t0, self.tape, self.start = seed, lane0, t0, tape, start
        nt = self.nt = ol.max_threads()
        o = self.o
        st = self.st = o.new_state(n)
        self.ob0 = o.batch_reset(st, seed, lane0, t0, nthreads=nt)
        self.st0 = st.copy()
        if start is not None:
            st[:] = start
        self.begin = st.copy()
        done = np.zeros(n, np.uint8)
        rows, self.bad, self.pre, self.post = [], 0, {}, {}
        for k in range(steps):
            t = t0 + 1 + k
            a = ol.synthetic_actions(n, seed, lane0, t, o.n_actions, nthreads=nt) if tape is None else tape[k].astype(np.int32)
            if k in keep:
                self.pre[k] = st.copy()
            ob, rew, done, bad = o.batch_step(st, a, seed, lane0, t, auto_reset=True, done=done, nthreads=nt)
            if k in keep:
                self.post[k] = st.copy()
            self.bad += bad
            rows.append((a, ob, rew, done.copy()))
        self.action, self.ob, self.reward, self.done = (np.stack([r[i] for r in rows]) for i in range(4))
        self.a_next = ol.synthetic_actions(n, seed, lane0, t0 + 1 + steps, o.n_actions, nthreads=nt)
        self.oracle_s = time.time() - t_or

    def env(self, env, kw, **more):
        e = Ref.env(self, env, kw, **more)                   # reset() at t0: its observations and state against the oracle's
        if self.start is not None:
            e.set_state(torch.as_tensor(self.start.view(np.int32), device="cuda"))
            assert np.array_equal(np_(e.state).view(np.uint32), self.begin) and e.call_counter == self.t0 + 1
        return e

    def returns_after(self, discount, pitch, ks):
        """or_batch_collect_returns over ks[0] steps, then ks[1] more on the same statistics, ...: [(acc, cnt, state)]"""
        st = self.begin.copy()
        acc, cnt = self.ol.new_return_stats(self.n, pitch)
        out, t = [], self.t0 + 1
        for k in ks:
            self.o.batch_collect_returns(st, acc, cnt, discount, self.seed, self.lane0, t, k, nthreads=self.nt)
            t += k
            out.append((acc.copy(), cnt.copy(), st.copy()))
        return out


# ---- coverage, from the oracle's rows and states ---------------------------------------------------------------------------------
def cov_gate(r, kw):
    """StochasticRock: per lane position of a quad, [steps whose move was gated away, steps whose move acted], over the kept
    steps.  Gated away: a move that would have changed the position (not into the north, south or west wall; east always
    moves or leaves) after which the state is unchanged, reward 0, observation 0, not done.  Also the share gated away."""
    size = kw.get("board_size", 7)
    cnt = np.zeros((4, 2), np.int64)
    pos = np.arange(r.n) & 3                                 # lane0 is a multiple of 4
    for k in sorted(r.pre):
        a, c = r.action[k], r.o.batch_compact(r.pre[k])
        x, y = c[:, 0], c[:, 1]
        would_move = ((a == 0) & (y < size - 1)) | (a == 1) | ((a == 2) & (y > 0)) | ((a == 3) & (x > 0))
        same = (r.pre[k] == r.post[k]).all(axis=0)
        gated = would_move & same & (r.reward[k] == 0) & (r.ob[k] == 0) & (r.done[k] == 0)
        c2 = r.o.batch_compact(r.post[k])
        acted = would_move & ((r.done[k] != 0) | (c2[:, 0] != x) | (c2[:, 1] != y))
        assert not (gated & acted).any() and ((gated | acted) == would_move).all()
        cnt[:, 0] += np.bincount(pos[gated], minlength=4)
        cnt[:, 1] += np.bincount(pos[acted], minlength=4)
    assert (cnt > 0).all(), cnt
    share = cnt[:, 0].sum() / cnt.sum()
    # the oracle's own gate at this threshold: 1 - p_move of the moves, to 14 standard deviations of the smallest sample used
    assert cnt.sum() < 2000 or abs(share - (1 - kw.get("p_move", .8))) < 7 / np.sqrt(cnt.sum()), (share, cnt)
    return "gated/acted per quad lane=%s share_gated=%.4f" % (cnt.tolist(), share)


def cov_flee(r, kw):
    """Tag, one opponent: per lane position of a quad, [failed TAGs after which the opponent moved, after which it stayed];
    several opponents: TAGs that removed an opponent while another fled."""
    K = kw.get("num_opponents", 1)
    cnt = np.zeros((4, 2), np.int64)
    removed_and_fled = 0
    pos = np.arange(r.n) & 3
    for k in sorted(r.pre):
        a, c, c2 = r.action[k], r.o.batch_compact(r.pre[k]), r.o.batch_compact(r.post[k])
        failed = (a == 4) & (r.reward[k] == -10) & (r.done[k] == 0)
        moved = (c[:, 1:1 + K] != c2[:, 1:1 + K]).any(axis=1)
        assert (c[failed, 0] == c2[failed, 0]).all() and (c[failed, -1] == c2[failed, -1]).all()
        cnt[:, 0] += np.bincount(pos[failed & moved], minlength=4)
        cnt[:, 1] += np.bincount(pos[failed & ~moved], minlength=4)
        hit = (a == 4) & (r.reward[k] == 10) & (r.done[k] == 0) & (c2[:, -1] < c[:, -1])
        other = (c[:, 1:1 + K] != c[:, :1]) & (c[:, 1:1 + K] != c2[:, 1:1 + K])
        removed_and_fled += int((hit & other.any(axis=1)).sum())
    if K == 1:
        assert (cnt > 0).all(), cnt
        return "failed TAG moved/stayed per quad lane=%s" % cnt.tolist()
    assert removed_and_fled > 0 and cnt.sum(axis=0).min() > 0, (removed_and_fled, cnt)
    return "failed TAG moved/stayed=%s removed+fled=%d" % (cnt.sum(axis=0).tolist(), removed_and_fled)


def cov_network(r, kw):
    """Network, from the pre-states and actions of the first step after set_state() of uniform words"""
    M = kw["n_machines"]
    s, a = r.begin[0].astype(np.int64), r.action[0].astype(np.int64)
    nA = 2 * M + 1
    if M <= 10:                                              # the state table: every (machine set, action) pair
        seen = np.bincount(s * nA + a, minlength=(1 << M) * nA)
        assert len(seen) == (1 << M) * nA and (seen > 0).all(), (M, int((seen == 0).sum()))
        return "pairs=%d all seen (min %d lanes)" % (len(seen), seen.min())
    down = ~s & ((1 << M) - 1)
    for kb in range((M + 7) // 8):                           # every value of every byte the loop indexes nbf8 with
        bits = min(8, M - 8 * kb)
        seen = np.bincount((down >> 8 * kb) & 255, minlength=256)
        assert (seen[:1 << bits] > 0).all() and seen[1 << bits:].sum() == 0, (M, kb)
    ping, reboot = int((a == 2 * (M - 1)).sum()), int((a == 2 * M - 1).sum())
    n_up = np.zeros(r.n, np.int64)
    for i in range(M):
        n_up += (s >> i) & 1
    late = int(((n_up >= 6) & (a < 2 * M)).sum())            # draws 0 .. n_up - 1 the machines', draw n_up >= 6 the action's
    assert ping > 0 and reboot > 0 and late > 0, (M, ping, reboot, late)
    return "down bytes all seen, last machine ping=%d reboot=%d, action draw past the sixth=%d" % (ping, reboot, late)


COVERAGE = {"stochrock": cov_gate, "tag": cov_flee}


def uniform_words(M, n):
    return np.random.RandomState(M).randint(0, 1 << M, n, dtype=np.uint64).astype(np.uint32)[None, :]


# ---- s1: step() ----------------------------------------------------------------------------------------------------------------------
def run_steps(ol, env, kw, n, steps=6, start=None, seed=SEED, lane0=LANE0):
    t_start = time.time()
    r = Traj(ol, env, kw, n, steps, seed=seed, lane0=lane0, start=start, keep=range(steps) if env != "network" else ())
    e = r.env(env, kw)
    for k in range(steps):
        ctx = (env, kw, n, k)
        assert np.array_equal(np_(e.synthetic_actions()), r.action[k]), ctx
        ob, rew, done, _ = e.step(torch.as_tensor(r.action[k], device="cuda"))
        assert np.array_equal(np_(ob), r.ob[k]) and np.array_equal(np_(rew), r.reward[k]), ctx
        assert np.array_equal(np_(done), r.done[k].astype(bool)), ctx
        if k in r.post:
            assert np.array_equal(np_(e.state).view(np.uint32), r.post[k]), ctx
    assert np.array_equal(np_(e.state).view(np.uint32), r.st) and e.invalid_action_count() == 0
    assert e.call_counter == T0 + 1 + steps
    cov = "-"
    if env in COVERAGE and n >= GATE:
        cov = COVERAGE[env](r, kw)
    elif env == "network" and start is not None and n >= GATE:
        cov = cov_network(r, kw)
    paramcov(env, kw, "s1" + ("b" if start is not None else ""), n, cov, r.oracle_s, t_start)


S1 = [("stochrock", kw) for kw in ROCK + [ROCK_HALF]] + [("tag", kw) for kw in TAG + [TAG_HALF] + TAG_MULTI]


@pytest.mark.parametrize("n", [1027, GATE])
@pytest.mark.parametrize("env,kw", S1, ids=ids(S1))
def test_single_steps(oracle_lib, env, kw, n):
    """s1: six step() calls, row by row and state by state: one lane per thread on a ragged batch, and what the step launcher
    picks at 2^19 lanes (step_quad_kernel for StochasticRock, the pooled pass for Tag)."""
    run_steps(oracle_lib, env, kw, n)


@pytest.mark.parametrize("start", ["reset", "words"])
@pytest.mark.parametrize("n", [1027, GATE])
@pytest.mark.parametrize("kw", NET, ids=[kwid(kw) for kw in NET])
def test_network_single_steps(oracle_lib, kw, n, start):
    run_steps(oracle_lib, "network", kw, n, start=uniform_words(kw["n_machines"], n) if start == "words" else None)


# ---- s2 (+ s6): the quad gate ----------------------------------------------------------------------------------------------------
def run_gate(ol, env, kw, steps, returns=False, packed=False, start=None, n=GATE, seed=SEED, lane0=LANE0, surface="s2"):
    """collect_synthetic(steps) in columns at n lanes; with `returns`, collect_returns(steps) and five steps more on the same
    statistics (s6); with `packed`, the packed sink too — all against one oracle pass"""
    t_start = time.time()
    keep = (0, 1, steps - 1) if env in COVERAGE else ()
    r = Traj(ol, env, kw, n, steps, seed=seed, lane0=lane0, start=start, keep=keep)
    ctx = (env, kw, n, steps)
    e = r.env(env, kw)
    tr = e.collect_synthetic(steps)
    name = last_kernel()
    r.check_cols(e, tr, ctx)
    assert np.array_equal(np_(tr["action"][steps]), r.a_next), ctx
    assert name == fused_name(env, kw, n, steps), (ctx, name)
    if packed:
        e = r.env(env, kw)
        tr = e.collect_synthetic(steps, layout="packed")
        name = last_kernel()
        r.check_cols(e, e.decode_trajectory(tr), ctx + ("packed",))
        assert name == fused_name(env, kw, n, steps, "Packed"), (ctx, name)
    if returns:
        more = 5
        e = r.env(env, kw)
        stats = e.collect_returns(steps)
        name = last_kernel()
        want = r.returns_after(e._discount, stats.acc.shape[1], (steps, more))
        assert np.array_equal(want[0][2], r.st)
        for i, (acc, cnt, st) in enumerate(want):
            if i:
                e.collect_returns(more, stats=stats)
            assert np.array_equal(np_(stats.acc)[:, :n].view(np.uint64), acc[:, :n].view(np.uint64)), ctx + ("returns", i)
            assert np.array_equal(np_(stats.cnt)[:, :n], cnt[:, :n]) and np.array_equal(np_(e.state).view(np.uint32), st), ctx + ("returns", i)
        assert name == fused_name(env, kw, n, steps, "Returns"), (ctx, name)
        short = last_kernel()                                # five steps: below the table-driven loops' 16
        assert short == fused_name(env, kw, n, more, "Returns") or \
            env == "stochrock" and short.startswith("steps_kernel<%s, " % env_name(env, kw)) and short.endswith(", Returns>"), (ctx, short)
        assert e.call_counter == T0 + 1 + steps + more and e.invalid_action_count() == 0
    cov = "-"
    if env in COVERAGE:
        cov = COVERAGE[env](r, kw)
    elif start is not None:
        cov = cov_network(r, kw)
    paramcov(env, kw, surface + ("+s6" if returns else "") + ("+packed" if packed else "") + "[%d]" % steps, n, cov, r.oracle_s, t_start)
    return r


S2 = [("stochrock", kw, 24, True, False) for kw in ROCK] + [("stochrock", ROCK_HALF, 24, False, False), ("stochrock", ROCK15, 24, False, False)] + \
     [("tag", kw, 24, True, False) for kw in TAG] + [("tag", kw, 8, False, False) for kw in TAG] + [("tag", TAG_HALF, 24, False, False)] + \
     [("tag", kw, 24, False, False) for kw in TAG_MULTI] + [("tag", TAG63, 24, False, True), ("tag", TAG64, 24, False, False)]


@pytest.mark.parametrize("env,kw,steps,returns,packed", S2, ids=["%s%s-%d" % (c[0], kwid(c[1]), c[2]) for c in S2])
def test_quad_gate_columns_and_returns(oracle_lib, env, kw, steps, returns, packed):
    """s2 (and s6, and obs_cells = 63's packed sink) at 2^19 lanes: steps_quad_kernel<StochasticRockEnv<W>>, tag_steps_quad_kernel
    with its step table (24 steps, obs_cells < 64) and without (8 steps; obs_cells = 64 at 24), steps_kernel<TagEnv, 2, true>
    for several opponents."""
    r = run_gate(oracle_lib, env, kw, steps, returns=returns, packed=packed)
    assert r.done.any() or kw is ROCK15                      # (15 x 15: no exit within 24 steps of a fresh episode)
    if kw is TAG63:
        assert last_kernel().startswith("tag_steps_quad_kernel<true")
    if kw is TAG64:
        assert fused_name(env, kw, GATE, steps) == "tag_steps_quad_kernel<false>"


NET_NAMES = {1: "2, Columns, true", 2: "2, Columns, true", 3: "2, Columns, true", 4: "2, Columns, true", 8: "2, Columns, true",
             9: "2, Columns, true", 10: "2, Columns, true", 11: "2, Columns, false", 17: "3, Columns, false", 24: "3, Columns, false",
             25: "4, Columns, false", 32: "4, Columns, false"}


@pytest.mark.parametrize("start", ["reset", "words"])
@pytest.mark.parametrize("kw", NET, ids=[kwid(kw) for kw in NET])
def test_network_quad_gate(oracle_lib, kw, start):
    """s2, twelve steps at 2^19 lanes from reset() and from uniformly random machine sets; with the four configurations of NET4
    also s6 (the returns sink adds the float64 base - .1, not the column's float32)."""
    M = kw["n_machines"]
    assert fused_name("network", kw, GATE, 12) == "network_steps_quad_kernel<%s>" % NET_NAMES[M]
    run_gate(oracle_lib, "network", kw, 12, returns=kw in NET4, start=uniform_words(M, GATE) if start == "words" else None)


@pytest.mark.parametrize("n", [GATE, TIE_LANES])
@pytest.mark.parametrize("M", sorted(TIE_SEED))
def test_network_ties_in_the_fused_loops(oracle_lib, M, n):
    """A lane whose first step has a draw that its low words decide (the seeds and lanes of test_env_params_host), inside
    network_steps_quad_kernel<4 | 3, ...> and inside steps_kernel<NetworkEnv, ...>: the exact per-lane form, step_exact."""
    kw = dict(n_machines=M, problem_type=RING)
    ties = tie_lanes(M, TIE_SEED[M])
    assert len(ties) >= 1 and all(LANE0 <= lane < LANE0 + n for lane, _ in ties)
    r = run_gate(oracle_lib, "network", kw, 4, seed=TIE_SEED[M], n=n, surface="s2-ties=%d" % len(ties))
    assert last_kernel() == ("network_steps_quad_kernel<%d, Columns, false>" % ((M + 7) // 8) if n == GATE else "steps_kernel<NetworkEnv, 1, true>")
    assert r.seed == TIE_SEED[M] and r.lane0 == LANE0


# ---- s3, s4: below the gate ------------------------------------------------------------------------------------------------------
S3 = [("stochrock", kw, SMALL) for kw in ROCK] + [("tag", kw, SMALL) for kw in TAG] + [("network", kw, 4096 + 4) for kw in NET4]


@pytest.mark.parametrize("steps", [24, 8])
@pytest.mark.parametrize("env,kw,n", S3, ids=ids(S3))
def test_one_lane_per_thread_columns(oracle_lib, env, kw, n, steps):
    """s3: the one-lane loop (its time-shared blocks; 8 steps: the arithmetic / table-free step); Network on 4096 + 4 lanes"""
    run_gate(oracle_lib, env, kw, steps, n=n, surface="s3")
    assert last_kernel() == "steps_kernel<%s, 1, %s>" % (env_name(env, kw), "true" if n % 256 == 0 else "false")


S4 = [("stochrock", kw) for kw in ROCK] + [("tag", kw) for kw in TAG]


@pytest.mark.parametrize("env,kw", S4, ids=ids(S4))
def test_half_quad_packed(oracle_lib, env, kw):
    """s4: collect_synthetic(24, layout="packed") at 3 * 2^17 lanes"""
    t_start = time.time()
    n, steps = PAIR, 24
    r = Traj(oracle_lib, env, kw, n, steps, keep=(0, 1, steps - 1))
    e = r.env(env, kw)
    tr = e.collect_synthetic(steps, layout="packed")
    name = last_kernel()
    r.check_cols(e, e.decode_trajectory(tr), (env, kw, "packed"))
    assert name == fused_name(env, kw, n, steps, "Packed") and name.endswith(", Packed, 2>"), name
    paramcov(env, kw, "s4[24]", n, COVERAGE[env](r, kw), r.oracle_s, t_start)


# ---- s5: tapes ---------------------------------------------------------------------------------------------------------------------
S5 = [("stochrock", kw, 24) for kw in ROCK] + [("tag", kw, 24) for kw in TAG] + [("tag", kw, 8) for kw in TAG] + [("network", kw, 24) for kw in NET4]


@pytest.mark.parametrize("n", [GATE, RAGGED])
@pytest.mark.parametrize("env,kw,steps", S5, ids=["%s%s-%d" % (c[0], kwid(c[1]), c[2]) for c in S5])
def test_tape_packed(oracle_lib, env, kw, steps, n):
    """s5: collect_tape(layout="packed") on a tape with out-of-range bytes: the quad loops' tape readers at 2^19 (Tag's packed
    sink rides the half-quad form; 8 steps: the table-free loop), the general loop at 4099"""
    t_start = time.time()
    o = oracle_lib.OracleEnv(env, **kw)
    tape = random_tape(o, steps, n, 11 + steps)
    r = Traj(oracle_lib, env, kw, n, steps, tape=tape, keep=(0, 1, steps - 1) if env in COVERAGE and n >= GATE else ())
    e = r.env(env, kw)
    tr = e.collect_tape(torch.as_tensor(tape, device="cuda"), layout="packed")
    name = last_kernel()
    r.check_cols(e, e.decode_trajectory(tr, steps), (env, kw, n, steps, "tape"))
    assert r.bad == int((tape >= o.n_actions).sum()) > 0
    assert name == fused_name(env, kw, n, steps, "Packed", taped=True), name
    cov = COVERAGE[env](r, kw) if r.pre else "bad=%d" % r.bad
    paramcov(env, kw, "s5[%d]" % steps, n, cov, r.oracle_s, t_start)


# ---- s7: episodes played to their end -----------------------------------------------------------------------------------------------
S7 = [("stochrock", kw) for kw in ROCK] + [("tag", kw) for kw in TAG + TAG_MULTI]


@pytest.mark.parametrize("policy", ["synthetic", "tape"])
@pytest.mark.parametrize("n", [GATE, RAGGED])
@pytest.mark.parametrize("env,kw", S7, ids=ids(S7))
def test_finish_episodes(oracle_lib, env, kw, n, policy):
    """s7: finish_episodes(40) from a state with frozen lanes, packed and narrow rows and the returns statistics (booked by
    controller_restatement.book over the oracle's rows; at 4099 lanes also test_gpu_episodes.check_returns)"""
    t_start = time.time()
    k = 40
    p = Pair(oracle_lib, env, kw, n, LANE0, pre_steps=2, seed=SEED, t0=T0)
    tape = random_tape(p.o, k, n, 7) if policy == "tape" else None
    act = None if tape is None else torch.as_tensor(tape, device="cuda")
    snap = p.snapshot()
    t_or = time.time()
    rows, bad = p.oracle_rows(k, tape)
    oracle_s = time.time() - t_or
    want_st, want_done = p.st.copy(), p.done.copy()
    acc, cnt = oracle_lib.new_return_stats(n)
    was = snap[4].copy()
    for a, ob, rw, d in rows:
        live = was == 0
        cr.book(acc, cnt, live, np.where((a & 0xFF) < p.o.n_actions, rw.astype(np.float64), 0.0), d, float(p.e._discount))
        was = d
    quad = env == "stochrock" and n >= GATE
    codes = None
    for layout in ("packed", "narrow", "returns"):
        p.restore(snap)
        p.e._err.zero_()
        out = p.e.finish_episodes(k, actions=act, layout=layout)
        ctx = (env, kw, n, policy, layout)
        want_name = "%s<%s, %s%s>" % ("episodes_quad_kernel" if quad else "episodes_kernel", env_name(env, kw), layout.capitalize(),
                                      ", Tape" if tape is not None else "")
        assert last_kernel() == want_name, (ctx, last_kernel())
        if layout != "returns":
            check_rows(p, out, rows, ctx)
            if layout == "packed":
                codes = (np_(out["traj"]) >> 16) & 0xFF
        else:
            assert tgc.same_f64(np_(out.acc[:, :n]), acc), ctx
            assert np.array_equal(np_(out.cnt[:, :n]), cnt), ctx
            if n < GATE:
                check_returns(p, out, [(a, ob, rw, d, codes[s][:n]) for s, (a, ob, rw, d) in enumerate(rows)], snap[4], ctx)
        assert np.array_equal(np_(p.e.state).view(np.uint32), want_st) and np.array_equal(np_(p.e._done), want_done), ctx
        assert p.e.invalid_action_count() == bad and p.e.call_counter == snap[2] + k, ctx
    frozen0, finished = int(snap[4].astype(bool).sum()), int((want_done != 0).sum())
    # lanes frozen from the start and, at 2^19 lanes, episodes that ended inside the launch (4099 lanes of StochasticRock with
    # p_move = .4 finish none in 42 steps: seven acting moves east at the least)
    assert 0 < frozen0 <= finished and (frozen0 < finished or n < GATE)
    paramcov(env, kw, "s7-%s[40]" % policy, n, "frozen at start=%d at end=%d bad=%d" % (frozen0, finished, bad), oracle_s, t_start)


# ---- s8: controllers ---------------------------------------------------------------------------------------------------------------
class CtrlRun(tgc.Run):
    """test_gpu_controller.Run whose calls start at call counter T0 + 1 (its own start at 1)"""
    t1 = T0 + 1

    def reference(self, k, calls=1):
        st, done, node = self.st0.copy(), np.zeros(tgc.N, np.uint8), self.start.copy()
        acc, cnt = self.ol.new_return_stats(tgc.N)
        res, bad = [], 0
        for c in range(calls):
            packed, b = cr.run(self.o, st, done, node, self.action, self.nxt, k, tgc.SEED, tgc.LANE0, self.t1 + c * k, acc, cnt,
                               float(self.e._discount), nthreads=self.nt)
            bad += b
            res.append((packed, bad, st.copy(), done.copy(), node.copy(), acc.copy(), cnt.copy()))
        return res

    def rewind(self):
        tgc.Run.rewind(self)
        self.e.call_counter = self.t1

    def check(self, k, ref, layouts=("packed", "narrow", "returns")):
        N = tgc.N
        for layout in layouts:
            self.rewind()
            res = None
            for c, (packed, bad, st, done, node, acc, cnt) in enumerate(ref):
                ctx = (self.env, layout, c)
                if layout == "returns":
                    res = self.e.run_controller(self.ctrl, k, stats=res)
                    assert tgc.same_f64(np_(res.acc[:, :N]), acc) and np.array_equal(np_(res.cnt[:, :N]), cnt), ctx
                else:
                    res = self.e.run_controller(self.ctrl, k, layout=layout, out=res)
                    got = tgc.rows_of(res, k)
                    assert np.array_equal(got, packed), ctx + (np.argwhere(got != packed)[:4].tolist(),)
                assert last_kernel() == "controller_kernel<%s, %s>" % (self.kernel_env, layout.capitalize()), (ctx, last_kernel())
                assert np.array_equal(np_(self.e.state).view(np.uint32), st), ctx
                assert np.array_equal(np_(self.e._done), done) and np.array_equal(np_(self.ctrl.node), node), ctx
                assert self.e.invalid_action_count() == bad and self.e.call_counter == self.t1 + (c + 1) * k, ctx


S8 = [("stochrock", kw) for kw in ROCK] + [("tag", kw) for kw in TAG] + [("network", kw) for kw in NET4]


@pytest.mark.parametrize("env,kw", S8, ids=ids(S8))
def test_controllers(oracle_lib, monkeypatch, env, kw):
    """s8: run_controller(40) under a random 128-node controller on 4099 lanes, every layout, against the restatement"""
    t_start = time.time()
    for name, v in (("N", RAGGED), ("SEED", SEED), ("LANE0", LANE0)):
        monkeypatch.setattr(tgc, name, v)
    k = 40
    r = CtrlRun(oracle_lib, env, *tgc.random_tables(oracle_lib.OracleEnv(env, **kw)), **kw)
    r.kernel_env = env_name(env, kw)
    t_or = time.time()
    ref = r.reference(k)
    oracle_s = time.time() - t_or
    assert ref[0][1] == 0
    finished = int(ref[0][3].astype(bool).sum())
    # some lanes finish and freeze inside the call, but Network's (never done) and StochasticRock's at p_move = .4 (seven acting
    # moves east at the least: none of 4099 lanes gets there in 40 steps under a random controller)
    assert finished < RAGGED and (finished > 0 or env == "network" or kw.get("p_move") == .4)
    r.check(k, ref)
    paramcov(env, kw, "s8[40]", RAGGED, "finished=%d nodes visited=%d" % (finished, len(np.unique(ref[0][4]))), oracle_s, t_start)


# ---- s9: the planner ----------------------------------------------------------------------------------------------------------------
S9 = S8 + [("tag", kw) for kw in TAG_MULTI]
ROOTS, SIMS, DEPTH = 130, 96, 10


@pytest.mark.parametrize("env,kw", S9, ids=ids(S9))
def test_rollout_and_plan(oracle_lib, env, kw):
    """s9: rollout_kernel from roots two steps off their start states — every simulation's return (float64), length, first action,
    last observation and termination — then plan()'s action values and plan_step()'s real step"""
    t_start = time.time()
    ol = oracle_lib
    nt = ol.max_threads()
    sim_lane0 = LANE0 * SIMS
    assert (LANE0 + ROOTS) * SIMS < 1 << 32
    o = ol.OracleEnv(env, **kw)
    e = make_env(env, kw, batch_size=ROOTS, seed=SEED, lane_offset=LANE0)
    e.call_counter = T0
    st = o.new_state(ROOTS)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, SEED, LANE0, T0, nthreads=nt))
    for _ in range(2):
        a = ol.synthetic_actions(ROOTS, SEED, LANE0, e.call_counter, o.n_actions)
        o.batch_step(st, a, SEED, LANE0, e.call_counter, nthreads=nt)
        e.step(torch.as_tensor(a, device="cuda"))
    assert np.array_equal(np_(e.state).view(np.uint32), st)
    t = e.call_counter
    t_or = time.time()
    want = o.batch_rollout(st, SIMS, DEPTH, e._discount, SEED, sim_lane0, t, nthreads=nt)
    oracle_s = time.time() - t_or
    got = e.rollout(DEPTH, sims_per_root=SIMS, lane_offset=sim_lane0)
    assert np.array_equal(np_(got["ret"]).view(np.uint64), want["ret"].view(np.uint64)), (env, kw)
    for k in ("n_steps", "first_action", "last_ob"):
        assert np.array_equal(np_(got[k]), want[k]), (env, kw, k)
    assert np.array_equal(np_(got["terminated"]), want["terminated"].astype(bool))
    assert int(want["n_steps"].sum()) > ROOTS * SIMS and len(np.unique(want["first_action"])) > 1
    for real_step in (False, True):
        t = e.call_counter
        r = o.batch_rollout(st, SIMS, DEPTH, e._discount, SEED, sim_lane0, t, nthreads=nt)
        w = ol.plan_reduce(r["ret"], r["first_action"], ROOTS, SIMS, o.n_actions)
        if real_step:
            ob, rew, done, _, plan = e.plan_step(DEPTH, sims_per_root=SIMS)
        else:
            plan = e.plan(DEPTH, sims_per_root=SIMS)
        assert np.array_equal(np_(plan["sim_ret"]).view(np.uint64), r["ret"].view(np.uint64)), (env, kw, real_step)
        assert np.array_equal(np_(plan["sim_first_action"]), r["first_action"]), (env, kw, real_step)
        for k in ("q", "value"):
            assert np.array_equal(np_(plan[k]).view(np.uint64), w[k].view(np.uint64)), (env, kw, real_step, k)
        assert np.array_equal(np_(plan["visits"]), w["visits"]) and np.array_equal(np_(plan["best"]), w["best"]), (env, kw, real_step)
        if real_step:
            ob_o, rew_o, done_o, bad = o.batch_step(st, w["best"], SEED, LANE0, t + DEPTH, auto_reset=True, nthreads=nt)
            assert np.array_equal(np_(ob), ob_o) and np.array_equal(np_(rew), rew_o) and np.array_equal(np_(done), done_o.astype(bool))
            assert np.array_equal(np_(e.state).view(np.uint32), st) and e.invalid_action_count() == bad == 0
    paramcov(env, kw, "s9", ROOTS * SIMS, "sim steps=%d terminated=%d first actions=%d" % (
        int(want["n_steps"].sum()), int(want["terminated"].sum()), len(np.unique(want["first_action"]))), oracle_s, t_start)


# ---- s10: the heuristic loop ---------------------------------------------------------------------------------------------------------
S10 = [("stochrock", kw) for kw in ROCK] + [("tag", kw) for kw in TAG]


@pytest.mark.parametrize("env,kw", S10, ids=ids(S10))
def test_heuristic_loop(oracle_lib, env, kw):
    """s10: heuristic_steps(h, 24) then (h, 5) on 4096 + 1 lanes (use_heuristic=True for StochasticRock)"""
    t_start = time.time()
    n = 4096 + 1
    n_done = _heuristic_fused_vs_oracle(oracle_lib, env, kw, n, (24, 5), seed=SEED, lane0=LANE0, t0=T0)
    paramcov(env, kw, "s10[24+5]", n, "episodes ended=%d" % n_done, 0.0, t_start)


# ---- s11: the particle update ----------------------------------------------------------------------------------------------------------
S11 = S8


@pytest.mark.parametrize("R,P", [(1, 4), (3, 64)], ids=["1x4", "3x64"])
@pytest.mark.parametrize("env,kw", S11, ids=ids(S11))
def test_particle_update(oracle_lib, env, kw, R, P):
    """s11: the belief update as test_gpu_particles checks it (particles and survivor counts after every update against the
    restatement), at its two smallest shapes, at lane_offset 2^22 and a call counter above 2^33"""
    t_start = time.time()
    run_filter(env, kw, R, P, match_reward=True, use_done=True, lane_offset=LANE0 if R > 1 else 0, call_counter=T0)
    paramcov(env, kw, "s11", R * P, "-", 0.0, t_start)
