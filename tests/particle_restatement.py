"""CPU restatement of the particle-belief contract (include/pomdp_hip.h: pomdp_particle_init / pomdp_particle_update /
pomdp_plan_particles), written from the header's words on top of the oracle: proposals from OracleEnv.batch_reset /
batch_step(auto_reset=False), the resampling in numpy, planning from _batch_rollout + plan_reduce.  Shared by
test_particles_host.py and test_gpu_particles.py."""
import numpy as np

from oracle import oracle_lib as ol
from oracle.philox_ref import philox4x32_10

STREAM_PARTICLE = 8


def particle_words(seed, lane0, n, t):
    """w_j: word 0 of block 0 of stream PARTICLE at (seed, lane0 + j, t), j < n"""
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = (lane0 + np.arange(n, dtype=np.uint64)) & 0xFFFFFFFF
    ctr[:, 1] = t & 0xFFFFFFFF
    ctr[:, 2] = (t >> 32) & 0xFFFFFFFF
    ctr[:, 3] = STREAM_PARTICLE << 24
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, key)[:, 0].astype(np.uint64)


def resample(prop, match, filt, R, P, seed, lane0, t):
    """the per-root resampling of proposals `prop` (uint32 [words, R * P]) -> (particles, n_match); `filt`: the filtered roots"""
    out = prop.copy()
    n_match = np.full(R, -1, np.int32)
    w = particle_words(seed, lane0, R * P, t)
    for r in np.nonzero(filt)[0]:
        cols = slice(r * P, (r + 1) * P)
        s = np.nonzero(match[cols])[0]
        m = len(s)
        n_match[r] = m
        if m == 0:
            continue                                                  # depleted: every proposal kept, unfiltered
        j = np.nonzero(~match[cols])[0]
        k = (w[r * P + j] * np.uint64(m)) >> np.uint64(32)
        out[:, r * P + j] = prop[:, r * P + s[k.astype(np.int64)]]
    return out, n_match


def init(o, old, R, P, seed, lane0, t, ob=None, where=None, nthreads=4):
    """pomdp_particle_init: `old` (uint32 [words, R * P] or None) holds what roots with where[r] == 0 keep"""
    prop = o.new_state(R * P)
    pob = o.batch_reset(prop, seed, lane0, t, nthreads=nthreads)
    filt = np.ones(R, bool) if where is None else np.asarray(where) != 0
    match = np.ones(R * P, bool) if ob is None else pob == np.repeat(np.asarray(ob, np.int32), P)
    parts, n_match = resample(prop, match, filt, R, P, seed, lane0, t)
    if old is not None:
        keep = np.repeat(~filt, P)
        parts[:, keep] = old[:, keep]
    return parts, n_match


def update(o, parts, action, ob, reward, done, match_reward, R, P, seed, lane0, t, nthreads=4):
    """pomdp_particle_update(parts -> new parts): the proposals are a step of all R * P columns, action[r] repeated P times,
    done flags clear, no auto-reset"""
    action = np.asarray(action, np.int64)
    filt = (action >= 0) & (action < o.n_actions)
    prop = parts.copy()
    a = np.repeat(np.where(filt, action, 0), P).astype(np.int32)
    pob, prew, pdone, _ = o.batch_step(prop, a, seed, lane0, t, auto_reset=False, done=np.zeros(R * P, np.uint8), nthreads=nthreads)
    match = pob == np.repeat(np.asarray(ob, np.int32), P)
    if done is not None:
        match &= (pdone != 0) == np.repeat(np.asarray(done) != 0, P)
    if match_reward:
        rw = np.asarray(reward, o.reward_dtype)
        match &= prew.view(np.uint32) == np.repeat(rw.view(np.uint32), P)
    out, n_match = resample(prop, match, filt, R, P, seed, lane0, t)
    unf = np.repeat(~filt, P)
    out[:, unf] = parts[:, unf]                                       # roots with an out-of-range action: unchanged
    return out, n_match


def plan(o, parts, R, P, sims, depth, discount, seed, lane0, t0, all_actions=False, nthreads=4):
    """pomdp_plan_particles: rollouts over the R * P columns, sims / P each, then the reduction over R roots x sims"""
    r = ol._batch_rollout(o, parts, sims // P, depth, discount, seed, lane0, t0, all_actions, nthreads=nthreads)
    return ol.plan_reduce(r["ret"], r["first_action"], R, sims, o.n_actions), r
