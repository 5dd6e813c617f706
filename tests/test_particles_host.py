"""Particle beliefs without a GPU: the C ABI's declarations and argument checks, the kernels' resources, and the contract's CPU
restatement (tests/particle_restatement.py) checked against Bayes' rule on the oracle alone."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

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


def rock_check_posterior(o, real, action, ob, parts, n_match, P, min_groups):
    """The one-step check shared with the GPU suite.  `real` (uint32 [words, R]): the real states after the step in which root
    r CHECKed rock action[r] - 5 and observed ob[r]; `parts`: the root's particles after one update from the reset prior.
    Roots are grouped by their exact posterior P(ob | good) / (P(ob | good) + P(ob | bad)) (OracleEnv.batch_compute_prob on the
    real state with the rock's code forced to 2 / 0); every group of >= 30 roots must hold the posterior within five standard
    errors of its mean fraction of good particles.  Returns the largest |z|."""
    R = real.shape[1]
    assert (n_match >= 1).all(), n_match.min()
    s64 = lambda x: x[0].astype(np.uint64) | ((x[1].astype(np.uint64) << np.uint64(32)) if len(x) > 1 else np.uint64(0))
    sh = (8 + 2 * (np.asarray(action, np.int64) - 5)).astype(np.uint64)
    lik = []
    for code in (2, 0):
        s = (s64(real) & ~(np.uint64(3) << sh)) | (np.uint64(code) << sh)
        forced = np.stack([(s >> np.uint64(32 * w)).astype(np.uint32) for w in range(real.shape[0])])
        lik.append(o.batch_compute_prob(forced, action, ob))
    post = lik[0] / (lik[0] + lik[1])
    frac = (((s64(parts).reshape(R, P) >> sh[:, None]) & np.uint64(3)) == 2).mean(axis=1)
    key = np.round(post, 12)
    checked, zmax = [], 0.0
    for v in np.unique(key):
        sel = key == v
        n = int(sel.sum())
        if n < 30:
            continue
        se = frac[sel].std(ddof=1) / np.sqrt(n)
        z = abs(frac[sel].mean() - v) / se
        print("posterior %.6f: %d roots, mean %.6f, |z| %.2f" % (v, n, frac[sel].mean(), z))
        assert abs(frac[sel].mean() - v) < 5 * se, (v, n, frac[sel].mean(), se)
        checked.append(v)
        zmax = max(zmax, z)
    assert len(checked) >= min_groups and min(checked) < 0.2 and max(checked) > 0.8, checked
    return zmax


def _rock_posterior_case(kw, P):
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("rock", **kw)
    R, seed, real_seed, nt = 4096, 11, 5, ol.max_threads()
    real = o.new_state(R)
    real_ob = o.batch_reset(real, real_seed, 0, 0, nthreads=nt)
    parts, nm = pr.init(o, None, R, P, seed, 0, 0, ob=real_ob, nthreads=nt)
    assert (nm == P).all()
    a = (5 + np.arange(R) % (o.n_actions - 5)).astype(np.int32)
    ob, rew, done, _ = o.batch_step(real, a, real_seed, 0, 1, auto_reset=False, nthreads=nt)
    parts, nm = pr.update(o, parts, a, ob, None, None, False, R, P, seed, 0, 1, nthreads=nt)
    return o, real, a, ob, parts, nm


@pytest.mark.parametrize("P", [64, 252, 1000])
@pytest.mark.parametrize("kw,min_groups", [({}, 10), (dict(board_size=15, num_rocks=15), 20)], ids=["7-8", "15-15"])
def test_restatement_rock_one_check_gives_the_exact_posterior(kw, min_groups, P):
    """What one filter step means, against mathematics rather than against the kernel's twin: from reset() RockSample's
    particles are independent draws of the prior (each rock good with probability 1/2), so after ONE update under CHECK j the
    survivors are exact posterior samples and the redraws copy survivors: a root's fraction of particles with rock j good is
    an unbiased estimate of P(ob | good) / (P(ob | good) + P(ob | bad)).  Root r CHECKs rock r % K from the start cell, so
    every distance (every sensor efficiency) occurs.  The bound is five standard errors of the group's mean, nothing added.

    Do NOT extend this to several updates with a margin this tight.  Measured on this restatement (2048 roots x 256 particles,
    12 CHECKs of three near rocks, efficiency about 0.97): for exact posteriors 0.0012 / 0.0074 / 0.9926 the particle means
    were 0.085 / 0.050 / 0.941, three to four standard errors off.  That is a rejection filter's finite-P bias (a hypothesis
    that died out in a root cannot return), not a defect of the filter: there is nothing to fix.

    Seeds: particles 11, real env 5, lanes from 0, reset at t = 0 and the update at t = 1.  With them the restatement gives
    12 groups for (7,8) and 22 for (15,15), largest |z| 2.09 / 1.60 / 2.14 and 2.23 / 1.51 / 2.35 for P = 64 / 252 / 1000,
    smallest n_match 16; re-check on the CPU before changing them."""
    o, real, a, ob, parts, nm = _rock_posterior_case(kw, P)
    print(kw, P, "smallest n_match", nm.min())
    print(kw, P, "largest |z| %.2f" % rock_check_posterior(o, real, a, ob, parts, nm, P, min_groups))
