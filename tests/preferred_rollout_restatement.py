"""CPU restatement of the preferred-policy rollout contract (include/pomdp_hip.h: pomdp_rollout_preferred /
pomdp_plan_preferred), written from the header's words on top of the oracle, with no new C: the roots' statistics and history
sums are expanded to one column per simulation; per step the list comes from ol._batch_preferred, the pick from the ROLLOUT
word (oracle.philox_ref), the step from batch_step(auto_reset=False, done=...), the private copies from Belief.update /
HistorySums.append(auto_reset=False), the return from numpy float64 with separate multiply and add; ol.plan_reduce reduces.
Shared by test_preferred_host.py and test_gpu_preferred.py."""
import numpy as np

from oracle import oracle_lib as ol
from oracle.philox_ref import philox4x32_10

STREAM_ROLLOUT = 5


def rollout_words(seed, lane0, n, t0, k):
    """word k of stream ROLLOUT at (seed, lane0 + i, t0), i < n: element k % 4 of block k / 4, as or_batch_rollout builds it"""
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = (lane0 + np.arange(n, dtype=np.uint64)) & 0xFFFFFFFF
    ctr[:, 1] = t0 & 0xFFFFFFFF
    ctr[:, 2] = (t0 >> 32) & 0xFFFFFFFF
    ctr[:, 3] = (STREAM_ROLLOUT << 24) | (k >> 2)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, key)[:, k & 3].astype(np.uint64)


def reward_f64(o, action, reward):
    """the float64 reward the reference's callers add up.  Network's is (machines' sum) - .1 / - 2.5 (network.py:94-109), which
    the step's float32 column rounds: rebuilt from the integer sum and the action."""
    r = np.asarray(reward).astype(np.float64)
    if o.name != "network":
        return r
    n_mach = (o.n_actions - 1) // 2
    a = np.asarray(action)
    cost = np.where(a < 2 * n_mach, np.where(a % 2 == 1, 2.5, .1), 0.)
    return np.rint(r + cost) - cost


def is_rock(o):
    return o.name in ("rock", "stochrock")


def expand(o, belief, history, prev_ob, R, sims):
    """the roots' policy inputs, one PRIVATE column per simulation (np.repeat): -> (ol.Belief | None, ol.HistorySums, prev_ob)"""
    n = R * sims
    hs = ol.HistorySums(o, n)
    for f in ("size", "last_action", "last_ob"):
        getattr(hs, f)[:] = np.repeat(np.asarray(history[f], np.int32), sims)
    bel = None
    if is_rock(o):
        for f in ("total_sample", "total_move"):
            getattr(hs, f)[:] = np.repeat(np.asarray(history[f], np.int32), sims, axis=1)
        bel = ol.Belief(o, n)
        for f, dt in ol.Belief.FIELDS:
            getattr(bel, f)[:] = np.repeat(np.asarray(belief[f], dt), sims, axis=1)
    pob = np.repeat(np.asarray(prev_ob, np.int32), sims) if prev_ob is not None else np.zeros(n, np.int32)
    return bel, hs, np.ascontiguousarray(pob)


def check_ok(bel):
    """the test of rock.py:371 per (rock, simulation)"""
    return (bel.measured < 5) & (np.abs(bel.count) < 2) & (bel.prob_valuable > 0) & (bel.prob_valuable < 1)


def rollout(o, states, belief, history, prev_ob, R, P, sims, depth, discount, seed, lane0, t0, preferred=True, nthreads=4):
    """pomdp_rollout_preferred.  states: uint32 [words, R * P] (P = 1: the true states); belief / history: dicts of the roots'
    arrays ([K, R] / [R]); prev_ob int32 [R].  preferred=False picks from _generate_legal() through the same loop.
    -> the five per-simulation outputs plus "stats": what the tests assert about the inputs (lists at step 0, whether a
    simulation cleared a check_ok bit by its own CHECKs, whether one took the total > 0 => SAMPLE rule)."""
    n, per = R * sims, sims // P
    assert sims % P == 0 and states.shape[1] == R * P
    st = np.ascontiguousarray(states[:, np.arange(n) // per])
    bel, hs, pob = expand(o, belief, history, prev_ob, R, sims)
    rock = is_rock(o)
    ret, disc = np.zeros(n, np.float64), np.ones(n, np.float64)
    n_steps, first = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    last_ob, term = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    alive = np.ones(n, bool)
    frozen = np.zeros(n, np.uint8)                                     # what batch_step takes as `done`: lanes that stopped
    stats = dict(cleared_check_ok=0, sample_rule=0)
    ck0 = check_ok(bel) if rock else None
    for k in range(depth):
        if preferred:
            lists, lens = ol._batch_preferred(o, st, hs, bel)
        else:
            lists, lens = ol._batch_legal(o, st)
        if k == 0:
            stats["lists0"], stats["lens0"] = lists.copy(), lens.copy()
        alive &= lens > 0                                              # an empty list ends the simulation (BattleShip, every cell shot)
        if not alive.any():
            break
        frozen[~alive] = 1
        w = rollout_words(seed, lane0, n, t0, k)
        idx = (w * np.maximum(lens, 1).astype(np.uint64)) >> np.uint64(32)
        a = np.where(alive, lists[np.arange(n), idx.astype(np.int64)], 0).astype(np.int32)
        if rock and preferred:                                         # rock.py:301-313: [SAMPLE] alone, on a rock the history vouches for
            stats["sample_rule"] += int((alive & (lens == 1) & (lists[:, 0] == 4)).sum())    # all-bad gives [EAST], not [SAMPLE]
        ob, rew, done, _ = o.batch_step(st, a, seed, lane0, t0 + k, auto_reset=False, done=frozen.copy(), nthreads=nthreads)
        r = reward_f64(o, a, rew)
        term_k = disc * r
        ret = np.where(alive, ret + term_k, ret)
        disc = np.where(alive, disc * discount, disc)
        first = np.where(alive & (k == 0), a, first).astype(np.int32)
        n_steps = np.where(alive, k + 1, n_steps).astype(np.int32)
        last_ob = np.where(alive, ob, last_ob).astype(np.int32)
        term = np.where(alive, done, term).astype(np.uint8)
        # the private copies, on live lanes: one non-auto-reset step of pomdp_heuristic_steps.  A lane that stopped earlier is
        # marked done with a non-CHECK action and ob 0, which leaves its statistics alone; its history is never read again.
        act = np.where(alive, a, 0).astype(np.int32)
        obs = np.where(alive, ob, 0).astype(np.int32)
        dn = np.where(alive, done, 1).astype(np.uint8)
        if rock:
            bel.update(st, act, obs, dn, auto_reset=False)
        hs.append(pob, act, obs, dn, auto_reset=False)
        pob = np.ascontiguousarray(np.where(alive, ob, pob).astype(np.int32))
        alive &= done == 0
    if rock:
        stats["cleared_check_ok"] = int((ck0 & ~check_ok(bel)).any(axis=0).sum())
    return dict(ret=ret, n_steps=n_steps, first_action=first, last_ob=last_ob, terminated=term, stats=stats)


def plan(o, states, belief, history, prev_ob, R, P, sims, depth, discount, seed, lane0, t0, nthreads=4):
    """pomdp_plan_preferred: the rollout, then the reduction over R roots x sims simulations"""
    r = rollout(o, states, belief, history, prev_ob, R, P, sims, depth, discount, seed, lane0, t0, nthreads=nthreads)
    return ol.plan_reduce(r["ret"], r["first_action"], R, sims, o.n_actions), r


def prepare_roots(o, R, steps, seed, lane0, nthreads=4):
    """R roots as the GPU tests prepare them: reset() at call 0, then `steps` real heuristic-policy steps (calls 1 .. steps, no
    auto-reset) -> (states, belief dict | None, history dict, prev_ob, done of the last step)"""
    st = o.new_state(R)
    pob = np.ascontiguousarray(o.batch_reset(st, seed, lane0, 0, nthreads=nthreads))
    hs = ol.HistorySums(o, R)
    bel = ol.Belief(o, R) if is_rock(o) else None
    out = ol._batch_heuristic_steps(o, st, hs, bel, pob, steps, seed, lane0, 1, auto_reset=False, nthreads=nthreads)
    belief = None if bel is None else {f: getattr(bel, f).copy() for f, _ in ol.Belief.FIELDS}
    history = {f: getattr(hs, f).copy() for f in ("size", "last_action", "last_ob", "total_sample", "total_move")}
    return st, belief, history, pob, out["done"][-1]
