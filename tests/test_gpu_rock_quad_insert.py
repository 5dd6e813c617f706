"""RockSample's quad and half-quad loops (steps_quad_kernel) since the state changes by one masked insert of the table entry's
first word (rock.hip.h: RecWide::build, boards with at most eight rocks): scripted tapes against the C oracle.

The loop keeps the state word in a layout of its own — position byte on top, rock j's code at bit 5 + 2 j — and converts when
the launch loads and stores it; a move inserts the new nibble, a SAMPLE on a rock the code 1 (over a collected rock's 1 too).
A lane's script is picked by its index (lane % number of scripts), so one launch of the smallest batch the launcher gives a
loop (3 << 18 lanes: a quad per thread; (3 << 17) + 4096: half a quad) walks every script with thousands of lanes — rocks good
and bad alike.  Every row's (action, ob, reward, done) of every lane and the state each launch leaves are the oracle's; on
top of that the rows of the scripted cases must show the outcome the case is about (deterministic boards only):
  * a move in each direction from an interior cell, along each border without leaving, off the board across each border
    (east: +10, done; the others: -100, done), and from size - 2 to size - 1 in x and in y (the nibble's top value);
  * SAMPLE on every rock that has a cell of its own — good (+10), bad (-10) and collected (-100, done, the state as it was) — and
    off any rock; CHECK of that rock from its own cell (the saturated entry) before the SAMPLE and after it, and of every rock
    from the start cell.
Scripts longer than 16 rows take a second 16-row launch (the tape's rows are padded with CHECKs of rock 0).

Boards: every one-state-word board with at most eight rocks the constructor accepts — (7,8), (7,7), (4,3) and (2,1), the
smallest K — and (11,11), whose launch takes the popcount filter's kernel (steps_quad_popc_kernel, the lane step as it was;
the launcher reports both as steps_quad_kernel) and StochasticRock(7,8) at its own smallest batch.  RockSample(7,1) and
RockSample(15,8) do not exist: the reference's constructor assert (rock.py:101), and with it make_params and the oracle,
takes board 7 with 7 or 8 rocks and board 15 with 15 only — test_boards_outside_the_reference_are_refused pins that."""
import numpy as np
import pytest
import torch

from test_gpu_parity import make_env, np_

pytestmark = pytest.mark.gpu

STEPS = 16
LOOPS = {"quad": (3 << 18, ""), "half": ((3 << 17) + 4096, ", 2")}
SEED, LANE0 = 77015, 1 << 21
N, E, S, W, SAMPLE, CHECK0 = 0, 1, 2, 3, 4, 5


def path(src, dst):
    """moves from cell src to cell dst inside the board: x first, then y"""
    (x0, y0), (x1, y1) = src, dst
    return [E if x1 > x0 else W] * abs(x1 - x0) + [N if y1 > y0 else S] * abs(y1 - y0)


def scripts_of(size, K):
    """-> {name: action list} from a fresh episode's start cell (a lane that is done starts there again)"""
    from gym_pomdp_amd import tables
    _, (sx, sy), rocks = tables.ROCK_CONFIG[size]
    out = {}
    own = {}                                                 # cell -> the rock id stamped last (rock.py:110-111)
    for j, c in enumerate(rocks):
        own[tuple(c)] = j
    for j in range(K):
        if own[tuple(rocks[j])] == j:
            out["rock%d" % j] = path((sx, sy), rocks[j]) + [CHECK0 + j, SAMPLE, CHECK0 + j, SAMPLE]
    out["checks"] = [CHECK0 + j for j in range(K)]
    out["east"] = [E] * (size - sx)                          # ... size - 2 -> size - 1, then off the board: the exit
    out["north"] = [N] * (size - sy)
    out["south"] = [S] * (sy + 1)
    out["west"] = [W] * (sx + 1)
    out["interior"] = [E, E, N, W, S, E, S, W, N]            # (from board 7 on: every direction from a cell off the border)
    # along the north border to the corner, down the east border, then across it; along the south border and across it
    out["rim"] = [N] * (size - 1 - sy) + [E] * (size - 1 - sx) + [S] * min(1, size - 1) + [E]
    out["south_rim"] = [S] * sy + [E, E, W][:max(0, size - 1)] + [S]
    out["sample_off"] = [SAMPLE, E, SAMPLE] if (sx, sy) not in own and (sx + 1, sy) not in own else [SAMPLE]
    return out


def tapes_of(scripts, n):
    names = list(scripts)
    rows = -(-max(len(s) for s in scripts.values()) // STEPS) * STEPS
    tape = np.full((rows, n), CHECK0, np.uint8)
    for i, nm in enumerate(names):
        s = scripts[nm]
        tape[:len(s), i::len(names)] = np.asarray(s, np.uint8)[:, None]
    return names, [tape[r:r + STEPS] for r in range(0, rows, STEPS)]


def run_tapes(oracle_lib, env, kw, kernel, tapes):
    """reset, then one collect_tape per tape: every row of every launch and the state after it against the oracle.
    -> per row (action, ob, reward, done) of the oracle, the state words before the first launch"""
    from gym_pomdp_amd import _native
    n = tapes[0].shape[1]
    nt = oracle_lib.max_threads()
    e = make_env(env, kw, batch_size=n, seed=SEED, lane_offset=LANE0)
    o = oracle_lib.OracleEnv(env, **kw)
    st = o.new_state(n)
    assert np.array_equal(np_(e.reset()), o.batch_reset(st, SEED, LANE0, 0, nthreads=nt))
    st0 = st.copy()
    done, t, rows = np.zeros(n, np.uint8), 1, []
    for tape in tapes:
        assert tape.shape == (STEPS, n) and int(tape.max()) < o.n_actions
        cols = e.decode_trajectory(e.collect_tape(torch.as_tensor(tape, device="cuda"), layout="packed"), STEPS)
        assert _native.lib().pomdp_last_fused_kernel().decode() == kernel, _native.lib().pomdp_last_fused_kernel()
        for k in range(STEPS):
            a = tape[k].astype(np.int32)
            ob, rew, done, bad = o.batch_step(st, a, SEED, LANE0, t, auto_reset=True, done=done, nthreads=nt)
            ctx = (env, kw, kernel, t)
            t += 1
            assert bad == 0
            assert np.array_equal(np_(cols["action"][k]), a), ctx
            assert np.array_equal(np_(cols["ob"][k]), ob), ctx
            assert np.array_equal(np_(cols["reward"][k]), rew), ctx
            assert np.array_equal(np_(cols["done"][k]), done.astype(bool)), ctx
            rows.append((a, ob.copy(), rew.copy(), done.copy()))
        assert np.array_equal(np_(e.state).view(np.uint32), st), (env, kw, kernel)      # the store's conversion
    assert e.invalid_action_count() == 0
    return rows, st0


def check_outcomes(size, K, scripts, names, rows, st0):
    """the rows each script is about, on a deterministic board: `rows` are the oracle's (and, by run_tapes, the kernel's)"""
    P = len(names)

    def row(nm, k):
        a, ob, rew, done = rows[k]
        i = names.index(nm)
        assert (a[i::P] == scripts[nm][k]).all()
        return ob[i::P], rew[i::P], done[i::P]

    for nm in names:
        s = scripts[nm]
        if nm.startswith("rock"):
            j, L = int(nm[4:]), len(s) - 4
            for k in range(L):                                                   # the walk stays inside
                ob, rew, done = row(nm, k)
                assert not ob.any() and not rew.any() and not done.any(), (nm, k)
            code = (st0[0][names.index(nm)::P] >> (8 + 2 * j)) & 3              # the fresh episode's rock: 0 bad, 2 good
            assert set(np.unique(code)) == {0, 2}, nm
            ob, rew, done = row(nm, L)                                           # CHECK on the rock's cell: always right
            assert np.array_equal(ob, np.where(code == 2, 2, 1)) and not rew.any() and not done.any(), nm
            ob, rew, done = row(nm, L + 1)                                       # SAMPLE: good +10, bad -10
            assert np.array_equal(rew, np.where(code == 2, 10, -10)) and not ob.any() and not done.any(), nm
            ob, rew, done = row(nm, L + 2)                                       # CHECK of the collected rock: not good
            assert (ob == 1).all() and not rew.any() and not done.any(), nm
            ob, rew, done = row(nm, L + 3)                                       # SAMPLE on the collected rock: 1 over 1
            assert (rew == -100).all() and done.all() and not ob.any(), nm
        elif nm == "checks":
            for k in range(K):
                ob, rew, done = row(nm, k)
                assert set(np.unique(ob)) == {1, 2} and not rew.any() and not done.any(), (nm, k)
        elif nm in ("east", "north", "south", "west", "rim", "south_rim"):
            for k in range(len(s) - 1):
                ob, rew, done = row(nm, k)
                assert not ob.any() and not rew.any() and not done.any(), (nm, k)
            ob, rew, done = row(nm, len(s) - 1)
            assert (rew == (10 if s[-1] == E else -100)).all() and done.all() and not ob.any(), nm
        elif nm == "interior" and size >= 7:
            for k in range(len(s)):
                ob, rew, done = row(nm, k)
                assert not ob.any() and not rew.any() and not done.any(), (nm, k)
        elif nm == "sample_off":
            for k in [i for i, a in enumerate(s) if a == SAMPLE]:
                ob, rew, done = row(nm, k)
                assert (rew == -100).all() and done.all() and not ob.any(), (nm, k)


BOARDS = {"7-8": dict(), "7-7": dict(board_size=7, num_rocks=7), "4-3": dict(board_size=4, num_rocks=3),
          "2-1": dict(board_size=2, num_rocks=1), "11-11": dict(board_size=11, num_rocks=11)}


@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("board", list(BOARDS))
def test_scripted_tapes_against_the_oracle(oracle_lib, board, loop):
    size, K = (int(v) for v in board.split("-"))
    n = LOOPS[loop][0]
    scripts = scripts_of(size, K)
    if board == "7-8":
        assert sorted(nm for nm in scripts if nm.startswith("rock")) == ["rock%d" % j for j in range(8)]
    names, tapes = tapes_of(scripts, n)
    assert len(tapes) == (2 if size == 11 else 1)
    # (RockSample(11,11): more than RockEnv::RESET_NUMERIC_K rocks, the launcher takes steps_quad_popc_kernel under this name)
    rows, st0 = run_tapes(oracle_lib, "rock", BOARDS[board], "steps_quad_kernel<RockEnv<1>, Packed, Tape%s>" % LOOPS[loop][1], tapes)
    check_outcomes(size, K, scripts, names, rows, st0)


def test_scripted_tapes_on_stochastic_rock(oracle_lib):
    """The same scripts through StochasticRock's quad loop: the gate refuses one action in five, so a lane follows its script
    only by chance — the oracle's rows say what happened; among thousands of lanes per script every outcome still occurs."""
    n = 1 << 19                                                                   # QUAD_MIN_STOCHROCK (kernels_common.hip.h)
    scripts = scripts_of(7, 8)
    names, tapes = tapes_of(scripts, n)
    rows, _ = run_tapes(oracle_lib, "stochrock", {}, "steps_quad_kernel<StochasticRockEnv<1>, Packed, Tape>", tapes)
    samples = np.concatenate([rew[a == SAMPLE] for a, _, rew, _ in rows])
    assert {10, -10} <= set(np.unique(samples))                                   # (its penalty is no reward and never ends an episode)
    assert any(((a >= CHECK0) & (ob == 0)).any() for a, ob, _, _ in rows)         # a CHECK the gate refused reads nothing
    assert any((done & (a == E) & (rew == 10)).any() for a, _, rew, done in rows)


def test_boards_outside_the_reference_are_refused(oracle_lib):
    """RockSample(7,1) and RockSample(15,8) — one-word boards the insert layout would hold — are no boards of the reference
    (rock.py:101): neither the env nor the oracle builds them, so no launch can meet them."""
    for kw in (dict(board_size=7, num_rocks=1), dict(board_size=15, num_rocks=8)):
        with pytest.raises(AssertionError):
            make_env("rock", kw, batch_size=1024, seed=1)
        with pytest.raises(ValueError):
            oracle_lib.OracleEnv("rock", **kw)
