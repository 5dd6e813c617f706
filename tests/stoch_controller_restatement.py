"""CPU restatement of the stochastic controller contract (include/pomdp_hip.h: pomdp_stoch_controller_episodes), written from
the header's words on top of the oracle: controller_restatement's per-step loop over OracleEnv.batch_step(auto_reset=False,
done=...) with the action and the successor DRAWN — words 0 and 1 of block 0 of stream CONTROLLER at (seed, lane, t), the
candidate index a count of the row's thresholds the word exceeds.  Shared by test_stoch_controller_host.py and
test_gpu_stoch_controller.py."""
import numpy as np

from controller_restatement import book, code_reward, reward_code
from oracle import philox_ref

STREAM_CONTROLLER = 10


def draws(seed, lane0, n, t):
    """(u_a, u_n), uint32 [n] each: words 0 and 1 of philox_ref.stream_words(seed, lane0 + i, t, STREAM_CONTROLLER, 2) for every
    lane at once (the same counter and key, through the same philox4x32_10; test_stoch_controller_host.py compares the two)"""
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = (int(lane0) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    ctr[:, 1] = int(t) & 0xFFFFFFFF
    ctr[:, 2] = (int(t) >> 32) & 0xFFFFFFFF
    ctr[:, 3] = STREAM_CONTROLLER << 24
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], np.uint64)
    w = philox_ref.philox4x32_10(ctr, key)
    return w[:, 0].copy(), w[:, 1].copy()


def pick(u, thr):
    """the candidate index of every lane: the number of j with u > thr[j] (strict); u uint32 [n], thr uint32 [n, cand - 1]"""
    return (u.astype(np.uint64)[:, None] > thr.astype(np.uint64)).sum(axis=1).astype(np.int64)


def drawn_action_bytes(action, action_thr, node, u_a):
    """(the action byte of every lane, its node as a safe index, whether the lane stands on a node at all): the drawn candidate
    where that lies in [0, 255], else 255; 255 for a node outside [0, K)"""
    K = action.shape[0]
    q_ok = (node >= 0) & (node < K)
    q = np.where(q_ok, node, 0)
    a = np.where(q_ok, action[q, pick(u_a, action_thr[q])], -1)
    return np.where((a >= 0) & (a <= 255), a, 255), q, q_ok


def run(o, st, done, node, action, action_thr, nxt, next_thr, k, seed, lane0, t0, acc=None, cnt=None, discount=None, nthreads=4):
    """k steps of every lane under the controller in candidate form (action int [K, B], action_thr uint32 [K, B - 1], nxt int
    [K, n_obs, D], next_thr uint32 [K, n_obs, D - 1]); st (uint32 [words, n]), done (uint8 [n]), node (int64 [n]) and the
    statistics acc / cnt (if given) are updated in place.  -> (packed records uint32 [k, n], the number of refused entries live
    lanes met)"""
    action, nxt = np.asarray(action, np.int64), np.asarray(nxt, np.int64)
    K, n_obs, D = nxt.shape
    action_thr = np.asarray(action_thr, np.uint32).reshape(K, action.shape[1] - 1)
    next_thr = np.asarray(next_thr, np.uint32).reshape(K, n_obs, D - 1)
    n = st.shape[1]
    packed = np.zeros((k, n), np.uint32)
    bad = 0
    for s in range(k):
        u_a, u_n = draws(seed, lane0, n, t0 + s)
        live = done == 0
        byte, q, q_ok = drawn_action_bytes(action, action_thr, node, u_a)
        valid = q_ok & (byte < o.n_actions)
        ob, rw, d, b = o.batch_step(st, np.where(valid, byte, 255).astype(np.int32), seed, lane0, t0 + s, auto_reset=False,
                                    done=done, nthreads=nthreads)                 # `done` is updated in place
        assert b == int((live & ~valid).sum())                                   # untouched and counted; a frozen lane is not
        bad += b
        code = reward_code(o.name, rw)
        rec = byte | ((ob.astype(np.int64) & 0xFF) << 8) | (code << 16) | (d.astype(np.int64) << 24)
        rec = np.where(live & ~valid, byte, rec)                                  # (ob, reward, done) = (0, 0, 0)
        rec = np.where(~live, byte | (1 << 24), rec)                              # frozen: the drawn action byte, done
        packed[s] = rec.astype(np.uint32)
        stepped = live & valid
        in_cols = (ob >= 0) & (ob < n_obs)
        col = np.where(in_cols, ob, 0)
        to = np.where(in_cols, nxt[q, col, pick(u_n, next_thr[q, col])], -1)
        moves = stepped & (to >= 0) & (to < K)
        bad += int((stepped & ~moves).sum())                                      # the step stands, the node stays, counted
        node[moves] = to[moves]
        if acc is not None:
            book(acc, cnt, live, np.where(valid, code_reward(o.name, code), 0.0), d, discount)
    return packed, bad
