"""CPU restatement of the controller contract (include/pomdp_hip.h: pomdp_controller_episodes), written from the header's
words on top of the oracle: a per-step loop over OracleEnv.batch_step(auto_reset=False, done=...) with numpy gathers for the
action and the successor, the frozen-row and refused-entry rules, the packed records and the float64 returns bookkeeping in
the stated order.  Shared by test_controller_host.py and test_gpu_controller.py."""
import numpy as np

NETWORK_BASES = 68                    # Network's reward code = kind * 68 + base, reward = base - (0, .1, 2.5)[kind]
NETWORK_OFF = (0.0, .1, 2.5)


def reward_code(env, rw):
    """the packed record's reward code of the oracle's rewards: the int8 reward itself, or Network's table index"""
    if env != "network":
        return rw.astype(np.int64) & 0xFF
    r = rw.astype(np.float64)
    frac = r - np.floor(r)
    kind = np.where(frac < .25, 0, np.where(frac < .75, 2, 1))
    base = np.rint(r + np.asarray(NETWORK_OFF)[kind]).astype(np.int64)
    return kind * NETWORK_BASES + base


def code_reward(env, code):
    """the float64 reward a code stands for (what the returns sink adds up)"""
    code = np.asarray(code, np.int64) & 0xFF
    if env != "network":
        return code.astype(np.uint8).view(np.int8).astype(np.float64)
    return (code % NETWORK_BASES).astype(np.float64) - np.asarray(NETWORK_OFF)[np.minimum(code // NETWORK_BASES, 2)]


def action_bytes(action, node):
    """(the action byte of every lane, its node as a safe index, whether the lane stands on a node at all): action[node] where
    that lies in [0, 255], else 255; 255 for a node outside [0, K)"""
    K = len(action)
    q_ok = (node >= 0) & (node < K)
    q = np.where(q_ok, node, 0)
    a = np.where(q_ok, action[q], -1)
    return np.where((a >= 0) & (a <= 255), a, 255), q, q_ok


def book(acc, cnt, live, rw, d, discount):
    """one step of the returns sink: acc = ret | disc | ret_done | ret_sum (float64 [4, n]), cnt = episodes | steps"""
    ret, disc, ret_done, ret_sum = acc
    L = live
    ret[L] = ret[L] + disc[L] * rw[L]
    disc[L] = disc[L] * discount
    cnt[1][L] += 1
    B = L & (d != 0)
    ret_done[B] = ret[B]
    ret_sum[B] = ret_sum[B] + ret[B]
    cnt[0][B] += 1
    ret[B] = 0.0
    disc[B] = 1.0


def run(o, st, done, node, action, nxt, k, seed, lane0, t0, acc=None, cnt=None, discount=None, nthreads=4):
    """k steps of every lane under the controller (action int [K], nxt int [K, n_obs]); st (uint32 [words, n]), done (uint8 [n]),
    node (int64 [n]) and the statistics acc / cnt (if given) are updated in place.  -> (packed records uint32 [k, n], the
    number of refused entries live lanes met)"""
    action, nxt = np.asarray(action, np.int64), np.asarray(nxt, np.int64)
    K, n_obs = nxt.shape
    n = st.shape[1]
    packed = np.zeros((k, n), np.uint32)
    bad = 0
    for s in range(k):
        live = done == 0
        byte, q, q_ok = action_bytes(action, node)
        valid = q_ok & (byte < o.n_actions)
        ob, rw, d, b = o.batch_step(st, np.where(valid, byte, 255).astype(np.int32), seed, lane0, t0 + s, auto_reset=False,
                                    done=done, nthreads=nthreads)                 # `done` is updated in place
        assert b == int((live & ~valid).sum())                                   # untouched and counted; a frozen lane is not
        bad += b
        code = reward_code(o.name, rw)
        rec = byte | ((ob.astype(np.int64) & 0xFF) << 8) | (code << 16) | (d.astype(np.int64) << 24)
        rec = np.where(live & ~valid, byte, rec)                                  # (ob, reward, done) = (0, 0, 0)
        rec = np.where(~live, byte | (1 << 24), rec)                              # frozen: the action byte, done
        packed[s] = rec.astype(np.uint32)
        stepped = live & valid
        in_cols = (ob >= 0) & (ob < n_obs)
        to = np.where(in_cols, nxt[q, np.where(in_cols, ob, 0)], -1)
        moves = stepped & (to >= 0) & (to < K)
        bad += int((stepped & ~moves).sum())                                      # the step stands, the node stays, counted
        node[moves] = to[moves]
        if acc is not None:
            book(acc, cnt, live, np.where(valid, code_reward(o.name, code), 0.0), d, discount)
    return packed, bad
