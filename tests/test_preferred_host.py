"""Rollouts under the env's preferred-action policy without a GPU: the C ABI's declarations and argument checks, the new
kernels' resources, and the contract's CPU restatement (tests/preferred_rollout_restatement.py) checked against the oracle's own
rollout and preferred lists — including that the inputs test_gpu_preferred.py uses are not vacuous."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preferred_rollout_restatement as rr  # noqa: E402

NAMES = ("pomdp_rollout_preferred_workspace", "pomdp_rollout_preferred", "pomdp_plan_preferred")
# what test_gpu_preferred.py runs: (oracle env, kwargs, real heuristic steps before planning); seed and shape below
GPU_CASES = [("rock", {}, 6), ("rock", dict(board_size=15, num_rocks=15), 8), ("stochrock", {}, 6), ("tag", {}, 5)]
GPU_IDS = ["rock7x8", "rock15x15", "stochrock7x8", "tag"]
SEED, ROOTS, SIMS, DEPTH = 4242, 96, 1024, 64


def test_entry_points_are_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    from gym_pomdp_amd.envs.base import BatchedEnv
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    for sym in NAMES:
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in _native.SYMBOLS
        assert hasattr(_native.lib(), sym)
    assert "planner_preferred.hip" in _native.UNITS and "planner_common.hip.h" in _native.HEADERS
    assert int(re.search(r"#define POMDP_ABI_VERSION (\d+)", hdr).group(1)) == _native.ABI_VERSION == _native.lib().pomdp_abi_version()
    for fn in (BatchedEnv.rollout, BatchedEnv.plan, BatchedEnv.plan_step):
        ps = inspect.signature(fn).parameters
        assert ps["policy"].default == "uniform" and ps["history"].default is None


def _rock_params():
    from gym_pomdp_amd import _native
    p = _native.RockParams(size=7, num_rocks=8, start_x=0, start_y=3)
    for i in range(256):
        p.grid[i] = -1
    for i in range(32):
        p.thr[i] = 1 << 52
    return p


def test_bad_arguments_are_refused_before_any_launch():
    """Every check runs on the host: none of these calls reaches the GPU (fake device pointers are never dereferenced)."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    p = C.byref(_rock_params())
    X = 1 << 40                                                          # a fake, 16-byte aligned "device" address
    bel = _native.RockBelief(*[X] * 6)
    po = _native.PlanOut(q=X, visits=X, best=X, value=X, stride=13, reserved=0)

    def hist(max_size=-1):
        return _native.HistoryPtrs(X, X, X, X, X, X, X if max_size >= 0 else None, X if max_size >= 0 else None, max_size, 0)

    def roll(env=0, params=p, state=X, r=8, P=1, sims=64, depth=4, b=C.byref(bel), h=None, pob=X, ws=X, lane0=0, ret=X, fa=X):
        h = C.byref(hist()) if h is None else h
        return L.pomdp_rollout_preferred(env, params, state, r, P, sims, depth, .95, b, h, pob, ws, 7, lane0, 1, ret, None, fa, None,
                                         None, None)

    def plan(out=C.byref(po), h=None, r=8, **kw):
        h = C.byref(hist()) if h is None else h
        return L.pomdp_plan_preferred(0, p, X, r, kw.get("P", 1), kw.get("sims", 64), 4, .95, C.byref(bel), h, X, X, 7, 0, 1, X, X, out, None)

    assert roll(params=None) == roll(state=None) == roll(ret=None) == roll(fa=None) == -1
    assert roll(h=C.byref(hist(max_size=3))) == plan(h=C.byref(hist(max_size=3))) == -1     # a bounded history is refused
    assert roll(h=C.byref(hist(max_size=0))) == -1
    assert roll(b=None) == roll(pob=None) == roll(ws=None) == roll(ws=X + 8) == -1       # RockSample needs all four
    assert roll(P=0) == roll(P=3) == roll(P=128) == -1                                   # sims % P, sims >= P
    assert roll(lane0=2) == roll(r=-1) == roll(depth=-1) == roll(r=1 << 27) == -1
    assert roll(env=9) == -1
    assert plan(out=None) == -1 and plan(r=1 << 31) == -1
    assert roll(r=0) == 0 and plan(r=0) == 0                                             # nothing to do, nothing launched
    assert L.pomdp_rollout_preferred_workspace(0, p, 96, 1024) == 32 * 8 * 96 * 1024
    assert L.pomdp_rollout_preferred_workspace(1, p, 96, 1024) == 0


def test_preferred_kernels_keep_nothing_in_scratch_memory():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = kr.collect(units=["planner_preferred.hip"])
    mine = [r for r in rows if r["kernel"].startswith("rollout_preferred_kernel<")]
    assert len(mine) == 5, [r["kernel"] for r in rows]                  # RockSample x 2 words x stochastic or not, Tag
    bad = [(r["kernel"], r["scratch"]) for r in rows if r["scratch"] != "0"]
    assert not bad, bad


@pytest.mark.parametrize("name,kw", [("tiger", {}), ("network", {}), ("battleship", {})], ids=["tiger", "network", "battleship"])
def test_restatement_equals_the_uniform_rollout_where_the_preferred_list_is_the_legal_list(name, kw):
    from oracle import oracle_lib as ol
    o = ol.OracleEnv(name, **kw)
    R, sims, depth, seed, lane0, t0 = 37, 52, 40, 99, 8, (1 << 32) + 3
    st, bel, hist, pob, _ = rr.prepare_roots(o, R, 3, seed, 0)
    want = ol._batch_rollout(o, st, sims, depth, .95, seed, lane0, t0)
    for preferred in (True, False):
        got = rr.rollout(o, st, bel, hist, pob, R, 1, sims, depth, .95, seed, lane0, t0, preferred=preferred)
        for k in ("ret", "n_steps", "first_action", "last_ob", "terminated"):
            assert np.array_equal(got[k], want[k]), (name, preferred, k)
        assert got["ret"].tobytes() == want["ret"].tobytes()
    assert want["n_steps"].max() > 1


@pytest.mark.parametrize("case", range(len(GPU_CASES)), ids=GPU_IDS)
def test_gpu_inputs_are_not_vacuous(case):
    """The roots test_gpu_preferred.py plans from, rebuilt on the oracle: step 0 of the restatement picks from the list
    ol._batch_preferred returns for the roots; that list differs from the legal list on at least half of the roots; and, for
    the RockSample envs, some simulation clears a check_ok bit through its own CHECKs and some simulation takes the
    "total > 0, so SAMPLE" rule of rock.py:301-311.  No RockSample root has ended (its agent stands on the board)."""
    from oracle import oracle_lib as ol
    name, kw, prep = GPU_CASES[case]
    o = ol.OracleEnv(name, **kw)
    nt = ol.max_threads()
    st, bel, hist, pob, done = rr.prepare_roots(o, ROOTS, prep, SEED, 0, nthreads=nt)
    if rr.is_rock(o):
        assert not done.any()
    r = rr.rollout(o, st, bel, hist, pob, ROOTS, 1, SIMS, DEPTH, .95, SEED, 0, prep + 1, nthreads=nt)
    b0, h0, _ = rr.expand(o, bel, hist, pob, ROOTS, 1)
    lists, lens = ol._batch_preferred(o, st, h0, b0)
    l0, n0 = r["stats"]["lists0"], r["stats"]["lens0"]
    assert np.array_equal(l0[::SIMS], lists) and np.array_equal(n0[::SIMS], lens)
    assert np.array_equal(l0, np.repeat(lists, SIMS, axis=0))
    w = rr.rollout_words(SEED, 0, ROOTS * SIMS, prep + 1, 0)
    pick = l0[np.arange(ROOTS * SIMS), ((w * n0.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)]
    assert np.array_equal(r["first_action"], pick)
    legal, legal_len = ol._batch_legal(o, st)
    differ = (legal_len != lens) | (legal != lists).any(axis=1)
    assert differ.sum() * 2 >= ROOTS, int(differ.sum())
    if rr.is_rock(o):
        assert r["stats"]["cleared_check_ok"] >= 1
        assert r["stats"]["sample_rule"] >= 1
    assert r["n_steps"].max() == DEPTH and len(np.unique(r["first_action"])) > 1
