"""The constructors' own parameters on the host: what make_params() hands the kernels for every value tests/test_gpu_env_params.py
launches with, against what oracle_lib.env_args hands the oracle and against tables.network_neighbours; and the search for the
seeds under which a Network lane's first step after reset() has a draw decided by its low words (a tie), which that module's
tie cases launch with."""
import numpy as np
import pytest

from gym_pomdp_amd import tables
from gym_pomdp_amd.envs import network as net_env, rock as rock_env, tag as tag_env
from oracle import oracle_lib as ol, philox_ref as pref

P_MOVE = (.4, .5, .95)                        # StochasticRockEnv(p_move=...)
MOVE_PROB = (.3, .4, .5, .55)                 # TagEnv(move_prob=...)
SENSE = {.3: 1, .4: 1, .5: 1, .55: 0, .95: 0}  # gt (p <= .5: [U > thr]) / le
NETWORKS = [(1, 2), (2, 2), (3, 2), (4, 3), (8, 2), (9, 1), (10, 2), (11, 2), (17, 1), (24, 2), (25, 3), (32, 2)]

# the coordinates every launch of tests/test_gpu_env_params.py runs at
SEED, LANE0, T0 = 0x9E3779B97F4A7C15, 1 << 22, (1 << 33) + 5
# ... but for the tie cases: the smallest seed in 1, 2, 3, ... for which a lane of LANE0 .. LANE0 + 4095 has a tie at the first
# step after a reset() at T0 (tie_lanes below; test_tie_seeds_are_the_smallest_with_a_tie re-derives them)
TIE_LANES = 4096
TIE_SEED = {32: 1, 17: 1}


def oracle_threshold(env, **kw):
    a = ol.env_args(env, **kw)
    return (a[3] | a[4] << 32, a[5]) if env == "stochrock" else (a[2] | a[3] << 32, a[4])


@pytest.mark.parametrize("p", P_MOVE)
def test_stochrock_gate_equals_the_oracles(p):
    for kw in (dict(), dict(board_size=15, num_rocks=15)):
        prm = rock_env.make_params(stochastic=True, p_move=p, **kw)[0]
        assert (int(prm.act_thr), int(prm.act_gt)) == oracle_threshold("stochrock", p_move=p, **kw)
        assert int(prm.act_gt) == SENSE[p] and prm.stochastic == 1
        assert 0 < int(prm.act_thr) < 1 << 53
        if p == .5:
            assert int(prm.act_thr) == 1 << 52


def test_stochrock_default_gate_is_the_captured_threshold():
    prm = rock_env.make_params(stochastic=True)[0]
    assert (int(prm.act_thr), int(prm.act_gt)) == (tables.TAG_MOVE_THR, 0)
    assert int(rock_env.make_params()[0].stochastic) == 0


@pytest.mark.parametrize("p", MOVE_PROB)
@pytest.mark.parametrize("kw", [dict(), dict(num_opponents=2), dict(num_opponents=4), dict(obs_cells=63), dict(obs_cells=64)],
                         ids=["1", "2opp", "4opp", "cells63", "cells64"])
def test_tag_flight_equals_the_oracles(p, kw):
    prm = tag_env.make_params(move_prob=p, **kw)[0]
    assert (int(prm.move_thr), int(prm.move_gt)) == oracle_threshold("tag", move_prob=p, **kw)
    assert int(prm.move_gt) == SENSE[p]
    assert (prm.num_opponents, prm.obs_cells) == (kw.get("num_opponents", 1), kw.get("obs_cells", 29))
    if p == .5:
        assert int(prm.move_thr) == 1 << 52
    a = ol.env_args("tag", move_prob=p, **kw)
    assert a[:2] == [prm.num_opponents, prm.obs_cells]


def test_tag_default_flight_is_the_captured_threshold():
    prm = tag_env.make_params()[0]
    assert (int(prm.move_thr), int(prm.move_gt)) == (tables.TAG_MOVE_THR, 0)


def test_thresholds_order_as_their_probabilities():
    """P[U <= thr] = p in the le sense, P[U > thr] = p in the gt sense: thr / 2^53 is p or 1 - p to within one part in 2^50"""
    for p in sorted(SENSE):
        thr, sense = tables.bernoulli_threshold(p)
        assert sense == ("gt" if SENSE[p] else "le")
        assert abs(thr / 2.0 ** 53 - (1 - p if SENSE[p] else p)) < 2.0 ** -50


@pytest.mark.parametrize("M,topology", NETWORKS + [(2, 1), (3, 1), (4, 1), (32, 1), (31, 3)], ids=lambda v: str(v))
def test_network_masks_equal_the_neighbour_lists(oracle_lib, M, topology):
    prm, words, n_actions, n_obs = net_env.make_params(M, topology)
    nb = tables.network_neighbours(M, topology)
    assert (prm.n_machines, words, n_actions, n_obs) == (M, 1, 2 * M + 1, 3)
    assert oracle_lib.OracleEnv("network", n_machines=M, problem_type=topology).n_actions == 2 * M + 1
    deg = 0
    for i in range(32):
        want = sum(1 << j for j in set(nb[i])) if i < M else 0
        assert int(prm.nb_mask[i]) == want, (M, topology, i)
        assert want >> M == 0
        if i < M and len(nb[i]) > 2:
            deg |= 1 << i
    assert int(prm.deg_gt2_mask) == deg
    if topology != 3:
        assert deg == 0
        for i in range(M):                       # a ring: the machine before and the machine after, whatever M
            assert int(prm.nb_mask[i]) == 1 << (i + 1) % M | 1 << (i - 1) % M
    if M == 1:
        assert int(prm.nb_mask[0]) == 1          # its own only neighbour
    if (M, topology != 3) == (32, True):
        assert int(prm.nb_mask[31]) == 1 << 30 | 1 << 0 and int(prm.nb_mask[0]) == 1 << 31 | 1 << 1
        assert int(prm.nb_mask[30]) == 1 << 31 | 1 << 29
    assert (int(prm.fail_thr), int(prm.fail_nb_thr), int(prm.obs_thr)) == \
        (tables.NET_FAIL_THR, tables.NET_FAIL_NEIGHBOUR_THR, tables.NET_OBS_THR)


def test_network_rejects_what_does_not_fit_the_state_word():
    for M in (0, 33):
        with pytest.raises(ValueError):
            net_env.make_params(M, 2)


# ---- ties --------------------------------------------------------------------------------------------------------------------
def top16(seed, lane0, n, t, n_draws):
    """[n, n_draws]: the top 16 bits of each lane's first n_draws doubles of a step (network_step_words' Q_j), from the quads'
    shared blocks, all lanes at once"""
    lanes = np.arange(lane0, lane0 + n, dtype=np.uint64)
    nblk = (n_draws + 1) // 2
    ctr = np.zeros((n, nblk, 4), np.uint64)
    ctr[..., 0] = (lanes >> np.uint64(2))[:, None]
    ctr[..., 1], ctr[..., 2] = t & 0xFFFFFFFF, t >> 32
    ctr[..., 3] = (pref.STREAM_STEP << 24) | np.arange(nblk, dtype=np.uint64)[None, :]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    w = pref.philox4x32_10(ctr, key)[np.arange(n), :, (lanes & np.uint64(3)).astype(np.int64)].astype(np.uint32)   # [n, nblk]
    return np.stack([w >> 16, w & 0xFFFF], axis=2).reshape(n, 2 * nblk)[:, :n_draws]


def tie_lanes(M, seed, lane0=LANE0, t0=T0, n=TIE_LANES):
    """[(lane, draw)] of lanes lane0 .. lane0 + n - 1 at the first step after a reset() at t0: every machine is up, so draw j < M
    is machine j's under fail_thr (no neighbour has failed) and draw M the action's under obs_thr; a tie is a draw whose top
    16 bits equal its threshold's."""
    q = top16(seed, lane0, n, t0 + 1, M + 1)
    thr = np.full(M + 1, tables.NET_FAIL_THR >> 37, np.uint32)
    thr[M] = tables.NET_OBS_THR >> 37
    return [(lane0 + int(i), int(j)) for i, j in np.argwhere(q == thr[None, :])]


def test_top16_is_network_step_words():
    for M, seed, lane in ((32, 1, LANE0 + 5), (17, 3, LANE0 + 4094), (3, SEED, (1 << 32) - 1)):
        w = pref.network_step_words(seed, lane, T0 + 1, M + 1)
        assert np.array_equal(top16(seed, lane, 1, T0 + 1, M + 1)[0], w[0::2] >> 16)


@pytest.mark.parametrize("M", sorted(TIE_SEED))
def test_tie_seeds_are_the_smallest_with_a_tie(M):
    """... and the tie is one the step meets: a machine's draw, or the action's where the synthetic policy's action is no no-op;
    the words themselves by network_step_words"""
    for seed in range(1, TIE_SEED[M]):
        assert not tie_lanes(M, seed), (M, seed)
    ties = tie_lanes(M, TIE_SEED[M])
    assert len(ties) >= 1
    real = 0
    for lane, j in ties:
        w = pref.network_step_words(TIE_SEED[M], lane, T0 + 1, M + 1)
        thr = tables.NET_OBS_THR if j == M else tables.NET_FAIL_THR
        assert int(w[2 * j]) >> 16 == thr >> 37
        a = int(pref.synthetic_actions(TIE_SEED[M], lane, 1, T0 + 1, 2 * M + 1)[0])
        real += j < M or a < 2 * M
    assert real >= 1
    print("network M=%d: seed %d, tie (lane, draw): %s" % (M, TIE_SEED[M], ties))
