"""CPU restatement of the preferred-policy rollout contract (include/pomdp_hip.h: pomdp_rollout_preferred /
pomdp_plan_preferred), written from the header's words on top of the oracle, with no new C: the roots' statistics and history
sums are expanded to one column per simulation; per step the list comes from ol._batch_preferred, the pick from the ROLLOUT
word (oracle.philox_ref), the step from batch_step(auto_reset=False, done=...), the private copies from Belief.update /
HistorySums.append(auto_reset=False), the return from numpy float64 with separate multiply and add; ol.plan_reduce reduces.
Shared by test_preferred_host.py and test_gpu_preferred.py.
rollout(counters=True) counts the policy's branches; construct_roots builds roots that reach all of them."""
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


def rock_codes(o, st):
    """status + 1 of every rock (0 worthless, 1 collected, 2 valuable) from the packed states: int32 [K, n]"""
    v = st[0].astype(np.uint64)
    if st.shape[0] > 1:
        v = v | (st[1].astype(np.uint64) << np.uint64(32))
    return np.stack([(v >> np.uint64(8 + 2 * j)) & np.uint64(3) for j in range(o.n_actions - 5)]).astype(np.int32)


# counters over live simulation-steps (simulations for repeat_check / from_empty_history), all 0 where they do not apply
COUNTERS = ("repeat_check", "fallback", "fallback_check_of_closed", "all_bad_east", "sample_rule", "check_ok_cleared",
            "check_ok_set_again", "move_bit_up", "move_bit_down", "sample_bit_up", "sample_bit_down", "from_empty_history",
            "nan_prob", "corner_tag", "empty_history_all_five")
ROCK_COUNTERS = COUNTERS[:12]                                          # what the RockSample tests want >= 1 (nan_prob: == 0)
TAG_COUNTERS = ("corner_tag", "empty_history_all_five", "from_empty_history")
TAG_CORNERS = np.array([0, 9, 10, 19, 26, 28])                         # tile indices: rows 0 and 1 hold ten tiles, rows 2 - 4 three


def rollout(o, states, belief, history, prev_ob, R, P, sims, depth, discount, seed, lane0, t0, preferred=True, nthreads=4,
            counters=False):
    """pomdp_rollout_preferred.  states: uint32 [words, R * P] (P = 1: the true states); belief / history: dicts of the roots'
    arrays ([K, R] / [R]); prev_ob int32 [R].  preferred=False picks from _generate_legal() through the same loop.
    -> the five per-simulation outputs plus "stats": what the tests assert about the inputs (lists at step 0, whether a
    simulation cleared a check_ok bit by its own CHECKs, the steps that took the total > 0 => SAMPLE rule) and, with
    counters=True (half as much time again at 10^5 simulations; the outputs are the same), COUNTERS, which count the policy's
    branches over live simulation-steps:
      repeat_check              simulations that executed a CHECK of a rock they had CHECKed before (they read their own entry back)
      fallback                  steps whose list is _generate_legal() because the heuristic's own list was empty (rock.py:374).  The
                                oracle's routine does not say which way it went, so: the list equals the legal list AND holds a
                                CHECK of a rock whose check_ok test fails on the simulation's statistics — an action the heuristic
                                never emits (it lists [SAMPLE], [EAST], or moves and the CHECKs that pass the test)
      fallback_check_of_closed  of those, the steps that picked such a CHECK
      all_bad_east              steps whose list is [EAST] because no uncollected rock has total_move >= 0 (rock.py:347)
      sample_rule               steps whose list is [SAMPLE] (rock.py:301-313)
      check_ok_cleared / _set_again   (rock, step) pairs at which the step's CHECK turned the rock's check_ok test off / on
      move_bit_up / _down, sample_bit_up / _down   the same for total_move >= 0 and total_sample > 0
      from_empty_history        simulations whose root has size 0
      nan_prob                  NaN prob_valuable at the roots or after the last step (0 / 0: the reference raises there)
      corner_tag                Tag: steps whose simulation has a history, saw the opponent last (last_ob 29) and stands in a
                                corner (tag.py:236) — the branch's own condition; its list is asserted to be [TAG]
      empty_history_all_five    Tag: steps that listed all five actions because the simulation's history was empty"""
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
    stats = dict(cleared_check_ok=0, **{c: 0 for c in COUNTERS})
    ck0 = check_ok(bel) if rock else None
    ar = np.arange(n)
    count = rock and preferred and counters
    if count:
        K = o.n_actions - 5
        checked, repeated = np.zeros((K, n), bool), np.zeros(n, bool)
        stats["nan_prob"] = int(np.isnan(bel.prob_valuable).sum())
    if preferred and counters and (rock or o.name == "tag"):
        stats["from_empty_history"] = int((hs.size == 0).sum())
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
        if count:
            ck = check_ok(bel)
            uncollected = rock_codes(o, st) != 1
            legal, legal_len = ol._batch_legal(o, st)
            fb = alive & (legal_len == lens) & (legal == lists).all(axis=1) & (uncollected & ~ck).any(axis=0)
            chk = alive & (a >= 5)
            j = np.where(chk, a - 5, 0)
            stats["fallback"] += int(fb.sum())
            stats["fallback_check_of_closed"] += int((fb & chk & ~ck[j, ar]).sum())
            all_bad = ~(uncollected & (hs.total_move >= 0)).any(axis=0)
            stats["all_bad_east"] += int((alive & all_bad & (lens == 1) & (lists[:, 0] == 1)).sum())
            repeated |= chk & checked[j, ar]
            checked[j[chk], ar[chk]] = True
            mv0, sm0 = hs.total_move >= 0, hs.total_sample > 0
        if preferred and counters and o.name == "tag":
            agent = (st[0] & np.uint32(31)).astype(np.int64)              # tag.py:68-74 is_corner: tiles (0|9, 0|1) and (5|7, 4)
            corner = np.isin(agent, TAG_CORNERS)
            rule = alive & (hs.size != 0) & (hs.last_ob == 29) & corner
            assert not (rule & ~((lens == 1) & (lists[:, 0] == 4))).any()
            stats["corner_tag"] += int(rule.sum())
            stats["empty_history_all_five"] += int((alive & (hs.size == 0) & (lens == 5)).sum())
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
        if count:
            ck2 = check_ok(bel)
            stats["check_ok_cleared"] += int((ck & ~ck2).sum())
            stats["check_ok_set_again"] += int((~ck & ck2).sum())
            mv1, sm1 = hs.total_move >= 0, hs.total_sample > 0
            stats["move_bit_up"] += int((~mv0 & mv1).sum())
            stats["move_bit_down"] += int((mv0 & ~mv1).sum())
            stats["sample_bit_up"] += int((~sm0 & sm1).sum())
            stats["sample_bit_down"] += int((sm0 & ~sm1).sum())
        alive &= done == 0
    if count:
        stats["repeat_check"] = int(repeated.sum())
        stats["nan_prob"] += int(np.isnan(bel.prob_valuable).sum())
    if rock:
        stats["cleared_check_ok"] = int((ck0 & ~check_ok(bel)).any(axis=0).sum())
    return dict(ret=ret, n_steps=n_steps, first_action=first, last_ob=last_ob, terminated=term, stats=stats)


def plan(o, states, belief, history, prev_ob, R, P, sims, depth, discount, seed, lane0, t0, nthreads=4, counters=False):
    """pomdp_plan_preferred: the rollout, then the reduction over R roots x sims simulations"""
    r = rollout(o, states, belief, history, prev_ob, R, P, sims, depth, discount, seed, lane0, t0, nthreads=nthreads, counters=counters)
    return ol.plan_reduce(r["ret"], r["first_action"], R, sims, o.n_actions), r


BELIEF_SEED_OFFSET = 0x9E3779B97F4A7C15                                 # gym_pomdp_amd.particles: a ParticleBelief's default seed


def prepare_roots(o, R, steps, seed, lane0, nthreads=4, P=1):
    """R roots as the GPU tests prepare them: reset() at call 0, then `steps` real heuristic-policy steps (calls 1 .. steps, no
    auto-reset) -> (states, belief dict | None, history dict, prev_ob, done of the last step); with P > 1 a sixth item: the
    P particles per root of a ParticleBelief that was reset with the reset observation and updated with every step's action
    and observation (tests/particle_restatement.py), uint32 [words, R * P]"""
    st = o.new_state(R)
    pob = np.ascontiguousarray(o.batch_reset(st, seed, lane0, 0, nthreads=nthreads))
    ob0 = pob.copy()
    hs = ol.HistorySums(o, R)
    bel = ol.Belief(o, R) if is_rock(o) else None
    out = ol._batch_heuristic_steps(o, st, hs, bel, pob, steps, seed, lane0, 1, auto_reset=False, nthreads=nthreads)
    belief = None if bel is None else {f: getattr(bel, f).copy() for f, _ in ol.Belief.FIELDS}
    history = {f: getattr(hs, f).copy() for f in ("size", "last_action", "last_ob", "total_sample", "total_move")}
    if P == 1:
        return st, belief, history, pob, out["done"][-1]
    import particle_restatement as pr
    bseed = (seed + BELIEF_SEED_OFFSET) & 0xFFFFFFFFFFFFFFFF
    parts, _ = pr.init(o, None, R, P, bseed, lane0 * P, 0, ob=ob0, nthreads=nthreads)
    for k in range(steps):
        parts, _ = pr.update(o, parts, out["action"][k], out["ob"][k], None, None, False, R, P, bseed, lane0 * P, k + 1, nthreads=nthreads)
    return st, belief, history, pob, out["done"][-1], parts


FAR_SUMS = np.array([-70000, -2048, 2048, 70000], np.int32)


def construct_roots(o, cols, P, belief, history, prev_ob, seed):
    """Roots near every threshold the policy tests, made from prepared ones: the prepared states, last actions and
    observations are kept and the statistics overwritten.  The arguments are left alone (copies).  cols: the state columns
    the simulations start from, uint32 [words, R * P].  -> (belief | None, history, prev_ob)

    Every env: a quarter of the roots get an EMPTY history (size 0, last action / observation as a cleared history holds
    them).  Their sums are overwritten like the others', so that `size != 0` alone keeps [SAMPLE] away from them.

    Tag: four in ten of the other roots have just seen the opponent (last_ob 29), for the corner rule.

    RockSample, per rock and root:
      total_sample, total_move   from -3 .. 3 or, one in ten, +-2048 / +-70000
      measured                   from 0 .. 6 or, one in ten, 250
      count                      from -3 .. 3 or, one in ten, +-130
      prev_ob                    from 0 .. 2, per root
      closed rocks               three in ten of the rocks that are valuable (worthless) in EVERY column of the root get lkw
                                 (lkv) exactly 0 and the other likelihood 1.  A closed rock that agrees with the state is only
                                 ever CHECKed into 0 * x + positive, never 0 / 0.  prob_valuable is recomputed from the
                                 likelihoods as the reference does.
    One RockSample root in six is then CORNERED, which is what reaches the legal fallback of rock.py:374 on the large boards:
      - every rock's total_move is below 0, except the nearest uncollected rock's (0 or 1; its total_sample 0 or -1);
      - every rock fails the check_ok test by its count alone (count +-2, measured 0 .. 3).
    Such a root's simulations walk to that rock and find the heuristic's list empty there, so they pick from the legal
    list.  That list holds CHECKs of rocks whose check_ok bit is clear: one of them sets the bit again (count back to +-1),
    or sends the last total_move below 0 (all bad: [EAST])."""
    rng = np.random.default_rng(seed)
    R = len(history["size"])
    history = {k: np.array(v, np.int32) for k, v in history.items()}
    cleared = ol.HistorySums(o, 1)
    empty = rng.random(R) < .25
    history["size"][empty] = 0
    history["last_action"][empty] = cleared.last_action[0]
    history["last_ob"][empty] = cleared.last_ob[0]
    if not is_rock(o):
        if o.name == "tag":
            history["last_ob"][~empty & (rng.random(R) < .4)] = 29
        return None, history, None if prev_ob is None else np.array(prev_ob, np.int32)
    K = o.n_actions - 5

    def draw(lo, hi, far):
        return np.where(rng.random((K, R)) < .1, rng.choice(far, size=(K, R)), rng.integers(lo, hi + 1, size=(K, R))).astype(np.int32)
    history["total_sample"] = draw(-3, 3, FAR_SUMS)
    history["total_move"] = draw(-3, 3, FAR_SUMS)
    belief = {k: np.array(v) for k, v in belief.items()}
    belief["measured"] = draw(0, 6, np.array([250], np.int32))
    belief["count"] = draw(-3, 3, np.array([-130, 130], np.int32))
    first = np.ascontiguousarray(cols[:, ::P])                          # a root's first column: the true state, or particle 0
    target = ol.Belief(o, R).select_target(first)                       # fresh statistics: the nearest uncollected rock, -1 if none
    for r in np.flatnonzero((rng.random(R) < 1 / 6) & (target >= 0)):
        history["total_move"][:, r] = -rng.integers(1, 4, size=K)
        history["total_move"][target[r], r] = rng.integers(0, 2)
        history["total_sample"][target[r], r] = -rng.integers(0, 2)
        belief["count"][:, r] = rng.choice(np.array([-2, 2]), size=K)
        belief["measured"][:, r] = rng.integers(0, 4, size=K)
    codes = rock_codes(o, cols).reshape(K, R, P)
    close = rng.random((K, R)) < .3
    valuable, worthless = close & (codes == 2).all(axis=2), close & (codes == 0).all(axis=2)
    belief["lkv"] = np.where(valuable, 1., np.where(worthless, 0., belief["lkv"]))
    belief["lkw"] = np.where(valuable, 0., np.where(worthless, 1., belief["lkw"]))
    belief["prob_valuable"] = (.5 * belief["lkv"]) / ((.5 * belief["lkv"]) + (.5 * belief["lkw"]))
    return belief, history, rng.integers(0, 3, size=R).astype(np.int32)


def put_roots(e, hist, belief, history, prev_ob):
    """The GPU side of construct_roots: write the roots' policy inputs (numpy, as construct_roots returns them) into a
    gym_pomdp_amd env and its History, with the derived words recomputed — History.move_ok here, the side statistics'
    check_ok by env.set_belief."""
    import torch
    for f, t in (("size", hist._size), ("last_action", hist.last_action), ("last_ob", hist.last_ob)):
        t.copy_(torch.as_tensor(np.ascontiguousarray(history[f])))
    if belief is None:
        return
    ts, tm = np.ascontiguousarray(history["total_sample"]), np.ascontiguousarray(history["total_move"])
    hist.total_sample.copy_(torch.as_tensor(ts))
    hist.total_move.copy_(torch.as_tensor(tm))
    w = (1 << np.arange(ts.shape[0], dtype=np.int64))[:, None]
    mo = ((tm >= 0) * w).sum(axis=0) | (((ts > 0) * w).sum(axis=0) << 16)
    hist.move_ok.copy_(torch.as_tensor(mo.astype(np.uint32).view(np.int32)))
    hist.prev_ob.copy_(torch.as_tensor(np.ascontiguousarray(prev_ob)))
    e.set_belief({k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in belief.items()})
