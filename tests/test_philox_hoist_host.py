"""The quad-shared Philox block with round 3's product of word 0 taken from in front of the step loop — host only.

gym_pomdp_amd/csrc/philox.hip.h: a quad-per-thread loop draws its blocks with counter words 0 and 3 fixed for the launch and
words 1, 2 (the call counter) wave-uniform; after round 2 word 0 is d_hi ^ lo(M1 c2) ^ (k0 + W0), which does not depend on the
counter's low word, so M0 times it is computed once per stretch of steps that share the counter's high word (philox_hoist) and
philox4x32_10_fixed reads it.  The forms are device code, so they are restated here — philox_fixed, philox_hoist,
philox4x32_10_fixed, stretch_end and the loops' walk over stretches — and held against oracle/philox_ref.py's block."""
import numpy as np
import pytest

from oracle import philox_ref as pr

M0, M1, W0, W1, M32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox_fixed(c0, c3, k1):
    a = u64(M0) * u64(c0)
    d = u64(M1) * ((a >> u64(32)) ^ u64(c3) ^ u64(k1))
    return dict(a_lo=a & u64(M32), d_hi=d >> u64(32), d_lo=d & u64(M32))


def philox_hoist(f, c2, k0):
    x0 = f["d_hi"] ^ ((u64(M1) * u64(c2)) & u64(M32)) ^ ((u64(k0) + u64(W0)) & u64(M32))
    q = u64(M0) * x0
    return dict(f, q_hi=q >> u64(32), q_lo=q & u64(M32))


def philox_fixed_block(f, c1, c2, k0, k1):
    """philox4x32_10_fixed: rounds 1 and 2 on the call counter, round 3 with the hoisted product, seven plain rounds"""
    m = u64(M32)
    b = u64(M1) * u64(c2)
    u0 = (b >> u64(32)) ^ u64(c1) ^ u64(k0)
    c = u64(M0) * u0
    k0, k1 = (u64(k0) + u64(W0)) & m, (u64(k1) + u64(W1)) & m
    x2 = f["a_lo"] ^ (c >> u64(32)) ^ k1
    x1, x3 = f["d_lo"], c & m
    k0, k1 = (k0 + u64(W0)) & m, (k1 + u64(W1)) & m
    p1 = u64(M1) * x2
    x0, x2, x1, x3 = (p1 >> u64(32)) ^ x1 ^ k0, f["q_hi"] ^ x3 ^ k1, p1 & m, f["q_lo"]
    for _ in range(7):
        k0, k1 = (k0 + u64(W0)) & m, (k1 + u64(W1)) & m
        p0, p1 = u64(M0) * x0, u64(M1) * x2
        x0, x2, x1, x3 = (p1 >> u64(32)) ^ x1 ^ k0, (p0 >> u64(32)) ^ x3 ^ k1, p1 & m, p0 & m
    return np.stack(np.broadcast_arrays(x0, x1, x2, x3), -1).astype(np.uint32)


def hoisted(c0, c1, c2, c3, k0, k1, c2_of_product=None):
    f = philox_hoist(philox_fixed(c0, c3, k1), c2 if c2_of_product is None else c2_of_product, k0)
    return philox_fixed_block(f, c1, c2, k0, k1)


def plain(c0, c1, c2, c3, k0, k1):
    ctr = np.stack(np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3))), -1).astype(np.uint32)
    key = np.stack(np.broadcast_arrays(np.asarray(k0, dtype=np.uint64), np.asarray(k1, dtype=np.uint64)), -1).astype(np.uint32)
    return pr.philox4x32_10(ctr, key)


def key_edge_coordinates():
    """(quad, t, seed) of tests/test_gpu_key_edges.py's K1 / K2 / K3 for a batch of 3 * 2^18 lanes: the env's counter at the
    sixth step of a launch after reset(t0) and the policy's one step earlier, on both sides of the carry"""
    n = 3 << 18
    ks = [(0x9E3779B97F4A7C15, (1 << 32) - n, (1 << 32) - 7), (1 << 32, 1 << 22, 0xFFFFFFFEFFFFFFF9), ((1 << 64) - 1, 0, 0)]
    out = []
    for seed, lane0, t0 in ks:
        for lane in (lane0, lane0 + n - 4):
            for t in range(t0, t0 + 12):
                out.append((lane >> 2, t & ((1 << 64) - 1), seed))
    return out


@pytest.mark.parametrize("c3", [pr.STREAM_ACTION << 24, pr.STREAM_STEP << 24, (pr.STREAM_STEP << 24) | 2], ids=["action", "gate", "sensor"])
def test_the_hoisted_form_is_the_block(c3):
    quads, ts, seeds = (np.array(v, dtype=np.uint64) for v in zip(*key_edge_coordinates()))
    his, los = np.meshgrid(np.array([0, 1, M32 - 1, M32], dtype=np.uint64), np.array([0, 1, M32], dtype=np.uint64))
    rng = np.random.RandomState(18)
    r = lambda n: rng.randint(0, 1 << 32, n, dtype=np.uint64)
    N = 4096
    c0 = np.concatenate([quads, np.full(his.size, 0x3FFFFFFF, np.uint64), r(N)])
    c1 = np.concatenate([ts & u64(M32), los.ravel(), r(N)])
    c2 = np.concatenate([ts >> u64(32), his.ravel(), r(N)])
    k0 = np.concatenate([seeds & u64(M32), np.full(his.size, 0x7F4A7C15, np.uint64), r(N)])
    k1 = np.concatenate([seeds >> u64(32), np.full(his.size, 0x9E3779B9, np.uint64), r(N)])
    want = plain(c0, c1, c2, c3, k0, k1)
    assert np.array_equal(hoisted(c0, c1, c2, c3, k0, k1), want)
    # a product hoisted for one high word does not serve the next: every block differs (what the stretches are for)
    stale = hoisted(c0, c1, c2, c3, k0, k1, c2_of_product=(c2 + u64(1)) & u64(M32))
    assert (stale != want).any(axis=-1).all()
    stale = hoisted(c0, c1, c2, c3, k0, k1, c2_of_product=(c2 - u64(1)) & u64(M32))
    assert (stale != want).any(axis=-1).all()


def stretch_end(s, end, t_lo, unit=1):
    more = (0 - t_lo - 1) & M32
    if unit == 2:
        more |= 1
    return s + 1 + min(end - s - 1, more)


def segments(k, unit=1):
    """LoopPrio::segment<unit>: where the four priority segments of a k-step launch end"""
    t0, t1, t2 = max(k >> 4, 1), (3 * k) >> 4, (7 * k) >> 4
    ends = [k - t2, k - t1, k - t0, k]
    return [min((e + unit - 1) // unit * unit, k) for e in ends]


def walk(t0, k, unit):
    """The step loop as the kernels run it: per segment, stretches; per stretch, the products of the counter high words at its
    head (unit 2: one per parity of the step); -> per step, the high word its product was hoisted for"""
    used, s = [], 0
    for seg_end in segments(k, unit):
        while s < seg_end:
            end, his = seg_end, []
            for h in range(unit):
                t = (t0 + s + h) & ((1 << 64) - 1)
                his.append(t >> 32)
                end = stretch_end(s, end, t & M32, unit)
            assert s < end <= seg_end and (unit == 1 or s % 2 == 0)
            while s < end:
                for h in range(unit):
                    if s + h < end:
                        used.append(his[h])
                s += unit
    return used


@pytest.mark.parametrize("unit", [1, 2])
def test_every_step_of_a_launch_reads_the_product_of_its_own_high_word(unit):
    """the wrap at every step of launches of 1 .. 70 steps (and none at all), for the plain loops and the one unrolled by two"""
    for k in list(range(1, 70)) + [255, 256]:
        for w in list(range(0, k + 2)) + [1 << 20]:
            for hi in (1, M32):
                t0 = ((hi << 32) - w) & ((1 << 64) - 1)                      # the counter of step w has low word 0
                used = walk(t0, k, unit)
                assert used == [((t0 + s) & ((1 << 64) - 1)) >> 32 for s in range(k)], (k, w, hi, unit)
