"""Particle beliefs without a GPU: the C ABI's declarations and argument checks, the kernels' resources, and the contract's CPU
restatement (tests/particle_restatement.py) checked against Bayes' rule on the oracle alone."""
import ctypes as C
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import particle_restatement as pr  # noqa: E402

NAMES = ("pomdp_particle_init", "pomdp_particle_update", "pomdp_plan_particles")


def test_entry_points_are_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    for sym in NAMES:
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in _native.SYMBOLS
        assert hasattr(_native.lib(), sym)
    assert "particles.hip" in _native.UNITS
    assert _native.ABI_VERSION == 15 and _native.lib().pomdp_abi_version() == 15
    assert re.search(r"POMDP_STREAM_PARTICLE\s*=\s*8\b", hdr)
    assert re.search(r"POMDP_PARTICLE_MATCH_REWARD\s*=\s*1\b", hdr) and _native.PARTICLE_MATCH_REWARD == 1


def _rock_params():
    from gym_pomdp_amd import _native
    p = _native.RockParams(size=7, num_rocks=8, start_x=0, start_y=3)
    for i in range(256):
        p.grid[i] = -1
    for i in range(32):
        p.thr[i] = 1 << 52
    return p


def test_bad_arguments_are_refused_before_any_launch():
    """Every check runs on the host: none of these calls reaches the GPU (fake device pointers are never dereferenced)."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    p = C.byref(_rock_params())
    A, B, X = 1 << 40, 1 << 41, 1 << 42            # fake, non-overlapping "device" addresses
    R, P = 8, 64

    def upd(env=0, params=p, pin=A, pout=B, act=X, ob=X, rew=None, done=None, nm=X, r=R, n=P, flags=0, lane0=0):
        return L.pomdp_particle_update(env, params, pin, pout, act, ob, rew, done, nm, r, n, flags, 7, lane0, 1, None)

    def init(params=p, parts=A, nm=X, r=R, n=P, lane0=0, env=0):
        return L.pomdp_particle_init(env, params, parts, None, None, nm, r, n, 7, lane0, 0, None)

    assert upd(params=None) == init(params=None) == -1
    assert upd(pin=None) == upd(pout=None) == upd(act=None) == upd(ob=None) == upd(nm=None) == -1
    assert init(parts=None) == init(nm=None) == -1
    for bad_p in (6, 8192, 0, 2, 4100):
        assert upd(n=bad_p) == init(n=bad_p) == -1, bad_p
    assert upd(lane0=2) == init(lane0=6) == -1                          # lane0 % 4
    assert upd(r=1 << 26, n=256) == -1                                   # lane0 + R * P > 2^32
    assert upd(r=-1) == -1
    assert upd(pout=A) == -1                                             # aliased in / out
    assert upd(pout=A + 4 * R * P - 4) == -1                             # overlapping in / out
    assert upd(flags=_native.PARTICLE_MATCH_REWARD) == -1                # reward needed
    assert upd(flags=4) == -1
    assert upd(env=9) == init(env=9) == -1                               # unknown env
    assert upd(r=0) == init(r=0) == 0                                    # nothing to do, nothing launched
    out = _native.PlanOut(q=X, visits=X, best=X, value=None, stride=13, reserved=0)
    plan = lambda n=P, s=256, lane0=0, env=0: L.pomdp_plan_particles(env, p, A, R, n, s, 8, .95, 0, 7, lane0, 0, B, X,
                                                                        C.byref(out), None)
    assert plan(s=100) == plan(s=32) == plan(n=6) == plan(lane0=2) == plan(env=9) == -1


def test_particle_kernels_keep_nothing_in_scratch_memory():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = kr.collect(units=["particles.hip"])
    names = [r["kernel"] for r in rows]
    assert sum(1 for k in names if k.startswith("particle_kernel<") and k.endswith(", false>")) == 11      # update, per env type
    assert sum(1 for k in names if k.startswith("particle_kernel<") and k.endswith(", true>")) == 11       # init, per env type
    bad = [(r["kernel"], r["scratch"]) for r in rows if r["scratch"] != "0"]
    assert not bad, bad


def test_restatement_filters_tiger_like_bayes():
    """The contract, restated on the oracle alone: 1024 roots x 256 particles of Tiger, each root a fixed tiger door
    observed through LISTEN eight times.  For a root that heard the left door L times and the right one R times the fraction
    of particles with the tiger on the left estimates the posterior .85^L .15^R / (.85^L .15^R + .15^L .85^R); averaged
    over the roots of each (L, R) it lies within 4.5 standard errors (plus 0.01) of it."""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("tiger")
    R, P, seed, real_seed = 1024, 256, 11, 5
    real = o.new_state(R)
    real_ob = o.batch_reset(real, real_seed, 0, 0)
    parts, nm = pr.init(o, None, R, P, seed, 0, 0, ob=real_ob)
    assert (nm == P).all()                                               # Tiger's reset observation is always the same
    n_left = np.zeros(R, int)
    listen = 2
    for t in range(1, 9):
        a = np.full(R, listen, np.int32)
        ob, rew, done, _ = o.batch_step(real, a, real_seed, 0, t, auto_reset=False)
        n_left += ob == 0
        parts, nm = pr.update(o, parts, a, ob, None, None, False, R, P, seed, 0, t)
        assert (nm >= 1).all()
    L, Rn = n_left, 8 - n_left
    left = (parts[0].reshape(R, P) & 1) == 0                              # state bit 0: the tiger's door (0 = left)
    frac = left.mean(axis=1)
    checked = 0
    for l in np.unique(L):
        sel = L == l
        if sel.sum() < 20:
            continue
        post = .85 ** l * .15 ** (8 - l) / (.85 ** l * .15 ** (8 - l) + .15 ** l * .85 ** (8 - l))
        se = np.sqrt(post * (1 - post) / (sel.sum() * P)) + frac[sel].std() / np.sqrt(sel.sum())
        assert abs(frac[sel].mean() - post) < 4.5 * se + 0.01, (l, frac[sel].mean(), post)
        checked += 1
    assert checked >= 3
    assert Rn.sum() > 0
