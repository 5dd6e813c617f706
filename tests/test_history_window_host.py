"""The bounded History's window without a GPU: the record walk that test_gpu_history_window.py holds the kernels to
(history_window_restatement.window_sums) against the oracle's own use of its records, the ring contract's restatement
against that walk on the streams the GPU test runs, and the evidence that those streams tell a subtly wrong ring from a
right one — every mutant of the contract listed below departs from the records on them."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import history_window_restatement as hw  # noqa: E402

CASES = [(K, m) for K in sorted(hw.ROCK_KW) for m in hw.MAX_SIZES]
IDS = ["K%d-hist%d" % c for c in CASES]
N = hw.N_LANES
# what tells each mutant from the contract: the two sums, or (head_kept: a ring that starts anywhere still drops its
# oldest record first, so the sums stay right) the window read back as rows 0 .. size - 1
MUTANTS = {"no_subtract": "sums", "evict_newest": "sums", "short_window": "sums", "head_kept": "window", "bit7_dropped": "sums",
           "sums_kept": "sums"}


def _window_differs(win, hs, K):
    """a decoded window against the oracle's records, as the four things the sums take from a record"""
    obs, act, nxt = hs.rec
    if win["valid"].shape != act.shape:
        return True
    v = np.arange(act.shape[0])[:, None] < hs.size[None, :]
    if not np.array_equal(win["valid"], v):
        return True
    chk, good, bad, pbad = hw.canonical(K, obs, act, nxt)
    gchk = np.where((win["action"] >= 5) & (win["action"] < 5 + K), win["action"] - 5, -1)
    return bool(((gchk != chk) | ((win["next"] == 2) != good) | ((win["next"] == 1) != bad) | ((win["bad"] != 0) != pbad))[v].any())


@functools.lru_cache(maxsize=None)
def run_case(K, max_size, garbage):
    """the stream of the case through the oracle's records, the contract's restatement and every mutant, in step ->
    (cells in which the restatement departs from the records, {mutant: {"sums": cells, "window": steps}} up to the step
    that tells the mutant apart, largest |sum|)"""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("rock", **hw.ROCK_KW[K])
    hs = ol.HistorySums(o, N, max_size=max_size)
    ring = hw.Ring(K, N, max_size)
    muts = {m: hw.Ring(K, N, max_size, mutant=m) for m in hw.Ring.MUTANTS}
    seen = {m: dict(sums=0, window=0) for m in muts}
    clears = hw.clear_masks(N, max_size)
    wrong, largest = 0, 0
    for t, (obs, act, nxt, done, ar) in enumerate(hw.stream(K, N, hw.n_appends(max_size), garbage=garbage)):
        if t in clears:
            hs.clear(where=clears[t])
            for r in [ring] + list(muts.values()):
                r.clear(where=clears[t])
        hs.append(obs, act, nxt, done, auto_reset=ar)
        ts, tm = hw.window_sums(hs, K)
        largest = max(largest, int(np.abs(ts).max()), int(np.abs(tm).max()))
        for r in [ring] + list(muts.values()):
            r.append(obs, act, nxt, done, ar)
        wrong += int((ring.total_sample != ts).sum() + (ring.total_move != tm).sum() + (ring.size != hs.size).sum() +
                     (ring.last_action != hs.last_action).sum() + (ring.last_ob != hs.last_ob).sum())
        w = ring.window()
        wrong += int(_window_differs(w, hs, K))
        if not garbage:                                               # every field of every record, as it was appended
            v = w["valid"]
            wrong += int((w["action"] != hs.rec[1])[v].sum() + (w["next"] != hs.rec[2])[v].sum() + (w["bad"] != (hs.rec[0] == 1))[v].sum())
        for m, r in list(muts.items()):
            seen[m]["sums"] += int((r.total_sample != ts).sum() + (r.total_move != tm).sum())
            if MUTANTS.get(m) == "window":
                seen[m]["window"] += int(_window_differs(r.window(), hs, K))
            elif m == "raw_byte":                                      # (the contract's window was compared above)
                seen[m]["window"] += int(not np.array_equal(r.ring, ring.ring) or not np.array_equal(r.head, ring.head))
            if seen[m][MUTANTS.get(m, "sums")]:
                del muts[m]                                            # told apart: nothing more to learn from it
    return wrong, seen, largest


@pytest.mark.parametrize("K,max_size", CASES, ids=IDS)
@pytest.mark.parametrize("garbage", [False, True], ids=["valid", "garbage"])
def test_ring_restatement_equals_the_record_walk(K, max_size, garbage):
    """push / evict / clear / auto-reset as the contract states them keep the sums, size, last action / observation and
    the window equal to the oracle's records after every append — also when the caller appends values no env produces:
    a record leaves the sums with exactly what it entered them with"""
    wrong, _, largest = run_case(K, max_size, garbage)
    assert wrong == 0
    if max_size >= 63:
        assert largest >= 10, largest           # the env's own policy keeps the sums within +-2


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_streams_tell_every_mutant_from_the_contract(mutant):
    """Each departure from the contract shows on the valid streams, in every case in which it is a departure at all:
    max_size = 0 keeps one record, so there a window one row short (kept at one row: a ring has at least one) is the
    contract itself, `evict_newest` drops the only record either way and `head` never leaves row 0."""
    for K, max_size in CASES:
        if max_size == 0 and mutant in ("short_window", "evict_newest", "head_kept"):
            continue
        _, seen, _ = run_case(K, max_size, False)
        assert seen[mutant][MUTANTS[mutant]] > 0, (mutant, K, max_size, seen[mutant])
    print("mutant %s: caught by the %s in every case" % (mutant, MUTANTS[mutant]))


def test_the_unmasked_byte_departs_from_the_records_on_garbage_only():
    """A ring byte written as (uint8)(action | next_ob << 5 | bad << 7) from whatever int32 came in: equal to the contract on
    what the envs produce, and off the records once actions such as 37 (& 31: CHECK 0) or next observations such as 4
    (<< 5: bit 7) are appended — they enter the sums as nothing and leave them as a CHECK."""
    for K, max_size in CASES:
        _, seen, _ = run_case(K, max_size, False)
        assert seen["raw_byte"] == dict(sums=0, window=0), (K, max_size)
        _, seen, _ = run_case(K, max_size, True)
        assert seen["raw_byte"]["sums"] > 0, (K, max_size)


def _states(o, K, kw, n):
    """per rock j two batches of n equal states in which only rock j is left (valuable): the agent next to it (north or
    south of it, so that the move rule alone decides the list) and on it (the SAMPLE rule first); and the rocks that own
    their cell (RockSample(15,15) lists two rocks on (1, 2): the grid holds the later one)"""
    from gym_pomdp_amd import tables
    pos = tables.ROCK_CONFIG[kw["board_size"]][2]
    owner = {p: j for j, p in enumerate(pos)}
    out = []
    for j in range(K):
        x, y = pos[j]
        for ay in ((y - 1 if y > 0 else y + 1), y):
            v = x | (ay << 4) | (2 << (8 + 2 * j)) | sum(1 << (8 + 2 * k) for k in range(K) if k != j)
            st = o.new_state(n)
            for w in range(o.words):
                st[w, :] = (v >> (32 * w)) & 0xFFFFFFFF
            out.append((j, ay == y, 0 if ay < y else 2, owner[pos[j]] == j, st))
    return out


@pytest.mark.parametrize("K,max_size", [(1, 3), (8, 3), (8, 63), (15, 2), (15, 63)], ids=["K1-hist3", "K8-hist3", "K8-hist63", "K15-hist2", "K15-hist63"])
def test_record_walk_predicts_the_oracles_preferred_lists(K, max_size):
    """window_sums against history_total as the oracle itself uses it (rock_preferred, rock.py:303-349): with one rock left
    and every rock measured out, the list is [SAMPLE] iff the agent stands on the rock and total_sample > 0, else [EAST] iff
    total_move < 0, else the one direction towards the rock (or, standing on it, the legal actions)."""
    from oracle import oracle_lib as ol
    kw = hw.ROCK_KW[K]
    o = ol.OracleEnv("rock", **kw)
    hs = ol.HistorySums(o, N, max_size=max_size)
    b = ol.Belief(o, N)
    b.measured[:] = 5                                             # rock.py:370-372 adds no CHECK
    states = _states(o, K, kw, N)
    assert sum(owns for _, on, _, owns, _ in states if on) >= K - 1
    hit = np.zeros(4, np.int64)                                       # sample > 0 / <= 0 on the rock, move < 0 / >= 0 next to it
    steps = hw.stream(K, N, 3 * (max_size + 1) + 12)
    for t, (obs, act, nxt, done, ar) in enumerate(steps):
        hs.append(obs, act, nxt, done, auto_reset=ar)
        if t % 5 and t != len(steps) - 1:
            continue
        ts, tm = hw.window_sums(hs, K)
        mo = hw.move_ok_word(ts, tm)
        for j, on_rock, toward, owns, st in states:
            lists, lens = o.batch_preferred(st, hs, b)
            move_ok, sample_ok = (mo >> j) & 1 != 0, ((mo >> (16 + j)) & 1 != 0) & (hs.size > 0)
            legal, n_legal = o.batch_legal(st)
            want = np.full_like(lists, 0)
            wlen = np.ones(N, np.int32)
            if on_rock:
                take = sample_ok & owns
                want[:, 0] = np.where(take, 4, 1)
                fall = ~take & move_ok                               # no direction leads to the cell the agent stands on
                want[fall], wlen[fall] = legal[fall], n_legal[fall]
                hit[0] += int(take.sum()); hit[1] += int((~take).sum())
            else:
                want[:, 0] = np.where(move_ok, toward, 1)
                hit[2] += int((~move_ok).sum()); hit[3] += int(move_ok.sum())
            assert np.array_equal(lens, wlen), (t, j, on_rock)
            cols = np.arange(lists.shape[1])[None, :] < wlen[:, None]
            assert np.array_equal(lists[cols], want[cols]), (t, j, on_rock)
    assert (hit > 0).all(), hit
