"""History.append() / History.clear() of a bounded history driven directly (history_append_kernel, history_push,
history_clear_kernel) with the streams of tests/history_window_restatement.py, against the oracle's records: after every
append the lane's words, the ring read back as records, the two per-rock sums as a walk over the oracle's records, and the
derived word.  test_history_window_host.py shows, without a GPU, that these streams tell a subtly wrong ring from a right one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import history_window_restatement as hw  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(K, m) for K in sorted(hw.ROCK_KW) for m in hw.MAX_SIZES]
IDS = ["K%d-hist%d" % c for c in CASES]
N = hw.N_LANES


def np_(t):
    return t.detach().cpu().numpy()


def _pair(env, kw, max_size):
    import gym_pomdp_amd as gpa
    from oracle import oracle_lib as ol
    e = gpa.make({"rock": "Rock-v0", "tag": "Tag-v0"}[env], batch_size=N, seed=3, **kw)
    e.reset()
    h = gpa.History(e, max_size=max_size, observation=torch.zeros(N, dtype=torch.int32))
    return e, h, ol.HistorySums(ol.OracleEnv(env, **kw), N, max_size=max_size)


def _drive(env, kw, K, max_size, garbage):
    from gym_pomdp_amd import Transition
    e, h, hs = _pair(env, kw, max_size)
    W = max_size + 1
    clears = hw.clear_masks(N, max_size)
    dev = lambda a: torch.as_tensor(a, device=e.device)          # noqa: E731
    assert h.ring.shape == ((W, N) if K else (0, N)) and h.head.shape == (N,)
    largest, wrapped = 0, 0
    for t, (obs, act, nxt, done, ar) in enumerate(hw.stream(K, N, hw.n_appends(max_size), garbage=garbage)):
        if t in clears:
            h.clear(where=dev(clears[t]))
            hs.clear(where=clears[t])
        h.append(Transition(dev(obs), dev(act), None, dev(nxt), dev(done)), auto_reset=ar)
        hs.append(obs, act, nxt, done, auto_reset=ar)
        ctx = (env, K, max_size, t)
        size, head = np_(h._size), np_(h.head)
        for name, got in (("size", size), ("last_action", np_(h.last_action)), ("last_ob", np_(h.last_ob))):
            assert np.array_equal(got, getattr(hs, name)), ctx + (name,)
        assert int(size.max()) <= W and int(head.min()) >= 0 and int(head.max()) < W, ctx
        if not K:
            assert (head == 0).all(), ctx                         # no ring: nothing moves the head
            continue
        ts, tm = hw.window_sums(hs, K)
        gts, gtm = np_(h.total_sample), np_(h.total_move)
        assert np.array_equal(gts, ts), ctx + ("total_sample", int((gts != ts).sum()), "cells differ")
        assert np.array_equal(gtm, tm), ctx + ("total_move", int((gtm != tm).sum()), "cells differ")
        mo = np_(h.move_ok).astype(np.int64) & 0xFFFFFFFF
        want = hw.move_ok_word(ts, tm)
        assert np.array_equal(mo & 0xFFFF, want & 0xFFFF) and np.array_equal(mo >> 16, want >> 16), ctx + ("move_ok",)
        win = hw.decode_ring(np_(h.ring), head, size, W)
        robs, ract, rnxt = hs.rec
        v = np.arange(W)[:, None] < hs.size[None, :]
        assert np.array_equal(win["valid"], v), ctx
        if not garbage:                                               # every field, as it was appended
            for name, got, want in (("action", win["action"], ract), ("next", win["next"], rnxt), ("bad", win["bad"], robs == 1)):
                assert np.array_equal(got[v], want[v]), ctx + ("ring", name)
        chk, good, bad, pbad = hw.canonical(K, robs, ract, rnxt)
        gchk = np.where((win["action"] >= 5) & (win["action"] < 5 + K), win["action"] - 5, -1)
        for name, got, want in (("check", gchk, chk), ("next==2", win["next"] == 2, good), ("next==1", win["next"] == 1, bad),
                                ("observation==1", win["bad"] != 0, pbad)):
            assert np.array_equal(got[v], want[v]), ctx + ("ring", name, int((got != want)[v].sum()))
        largest = max(largest, int(np.abs(ts).max()), int(np.abs(tm).max()))
        wrapped = max(wrapped, int(((size == W) & (head == W - 1)).sum()))
    if K:
        assert wrapped > 0, "no lane's head reached the ring's last row"
        if max_size >= 63:
            assert largest >= 10, largest


@pytest.mark.parametrize("K,max_size", CASES, ids=IDS)
def test_window_equals_the_oracles_records_after_every_append(K, max_size):
    """what the envs' own transitions can be: actions 0 .. 4 + K, next observations 0 .. 2"""
    _drive("rock", hw.ROCK_KW[K], K, max_size, garbage=False)


@pytest.mark.parametrize("K,max_size", CASES, ids=IDS)
def test_window_takes_out_what_it_put_in_whatever_is_appended(K, max_size):
    """History.append() takes any int32: actions such as 37, 69 or -27 (& 31: CHECK 0), 5 + K, 1 << 20, INT32_MIN and next
    observations 3, 4, 5, -1 are no CHECK results — they enter neither sum and must not leave one when the ring drops them"""
    _drive("rock", hw.ROCK_KW[K], K, max_size, garbage=True)


@pytest.mark.parametrize("max_size", [0, 2])
def test_tag_history_has_no_ring(max_size):
    """Tag: no rocks, no ring — `size` saturates at max_size + 1 and `head` stays 0"""
    _drive("tag", {}, 0, max_size, garbage=False)
