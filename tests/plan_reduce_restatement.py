"""pomdp_plan_reduce's contract (include/pomdp_hip.h) restated in Python floats — chunks of 64 simulations by index,
simulation-index order within a chunk, chunk order across chunks, every sum from +0.0, best = the first strict maximum among
the visited actions — with the other summation orders a reduction might take, and the inputs test_plan_reduce_host.py and
test_gpu_plan_reduce_edges.py share."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ROOTS = 3
SHAPES = [(1, 1), (63, 2), (64, 3), (65, 3), (1023, 5), (1024, 1), (1025, 64), (2049, 65), (1100, 255)]       # (S, A)
ORDERS = ("contract", "sequential", "chunks32", "chunks128", "reversed")


def reduce(ret, first_action, R, S, A, order="contract"):
    """-> dict(q float64 [R, A], visits int32 [R, A], best int32 [R], value float64 [R]); Python floats are IEEE doubles
    added one at a time, so the order written here is the order taken"""
    chunk = {"contract": 64, "sequential": S, "chunks32": 32, "chunks128": 128, "reversed": 64}[order]
    ret, fa = np.asarray(ret, np.float64).reshape(R, S).tolist(), np.asarray(first_action, np.int64).reshape(R, S).tolist()
    out = dict(q=np.zeros((R, A), np.float64), visits=np.zeros((R, A), np.int32), best=np.zeros(R, np.int32), value=np.zeros(R, np.float64))
    for r in range(R):
        total, cnt = [0.0] * A, [0] * A
        for c0 in range(0, S, chunk):
            part = [0.0] * A
            js = range(c0, min(c0 + chunk, S))
            for j in (reversed(js) if order == "reversed" else js):
                a = fa[r][j]
                if 0 <= a < A:
                    part[a] = part[a] + ret[r][j]
                    cnt[a] += 1
            total = [x + y for x, y in zip(total, part)]
        b, bq = -1, 0.0
        for a in range(A):
            q = total[a] / float(cnt[a]) if cnt[a] > 0 else 0.0
            out["q"][r, a], out["visits"][r, a] = q, cnt[a]
            if cnt[a] > 0 and (b < 0 or q > bq):
                b, bq = a, q
        out["best"][r], out["value"][r] = b, (bq if b >= 0 else 0.0)
    return out


def shape_inputs(S, A, R=ROOTS, seed=20261018):
    """returns spread over thirteen decades, so that the order of the additions shows in the low bits; first actions uniform
    on [-1, A)"""
    rng = np.random.default_rng([seed, S, A])
    ret = rng.standard_normal(R * S) * 10.0 ** rng.integers(-6, 7, R * S)
    return ret, rng.integers(-1, A, R * S).astype(np.int32)


SPECIAL_S, SPECIAL_A = 130, 4
SPECIAL = ("tie", "negative", "nan_first", "nan_later", "negative_zero", "infinities", "nothing")


def special_roots():
    """one call, S = 130, A = 4 -> (ret [7 * 130], first_action [7 * 130]); root order: SPECIAL"""
    S, A = SPECIAL_S, SPECIAL_A
    j = np.arange(S)
    ret, fa = np.zeros((len(SPECIAL), S)), np.zeros((len(SPECIAL), S), np.int64)
    # actions 1 and 3 tie at exactly 2.5 (3: 2.0 and 3.0 in equal numbers), action 0 below them, action 2 never taken
    fa[0] = np.where(j < 2, 0, np.where(j % 2 == 0, 1, 3)); ret[0] = np.where(j < 2, 1.0, np.where(j % 2 == 0, 2.5, 2.0 + (j // 2) % 2))
    fa[1] = np.where(j % 3 == 0, 2, -1); ret[1] = -7.0                                     # one action, every return -7
    fa[2] = 1 + j % 3; ret[2] = np.where(fa[2] == 1, 1.0, 5.0); ret[2, 63] = np.nan        # NaN on the first visited action (1)
    fa[3] = np.where(j % 3 == 1, 2, j % 3 * 3 // 2); ret[3] = np.where(fa[3] == 0, 1.0, .5); ret[3, 1] = np.nan    # actions 0, 2 (NaN), 3
    fa[4] = j % 4; ret[4] = -0.0
    fa[5] = j % 4; ret[5] = j % 5; ret[5, 1] = np.inf; ret[5, 65] = -np.inf                # both on action 1, in different chunks
    fa[6] = np.array([-1, A, 255, 256, INT32_MIN])[j % 5]; ret[6] = 1.0 + j
    assert np.count_nonzero(fa[0] == 1) == 64 and np.count_nonzero((fa[0] == 3) & (ret[0] == 2.0)) == np.count_nonzero((fa[0] == 3) & (ret[0] == 3.0))
    return ret.reshape(-1), fa.reshape(-1).astype(np.int32)


def out_of_range_inputs(A, S=200, seed=7):
    """one root: valid first actions mixed with values at or beyond A that are not -1 — A itself, the kernel's byte marker
    255, 256 + a for a valid a (its low byte is a valid action), INT32_MAX, INT32_MIN: each counts for no action
    -> (ret, first_action, number of simulations that count)"""
    rng = np.random.default_rng([seed, A])
    fa = rng.integers(0, A, S).astype(np.int64)
    bad = np.array([A, 255, 256 + int(rng.integers(0, A)), 256, INT32_MAX, INT32_MIN, -1], np.int64)
    assert ((bad < 0) | (bad >= A)).all()
    out = rng.random(S) < .4
    fa = np.where(out, bad[rng.integers(0, len(bad), S)], fa)
    fa[:len(bad)] = bad                                                                    # each of them at least once
    out[:len(bad)] = True
    return rng.standard_normal(S), fa.astype(np.int32), int((~out).sum())
