#!/usr/bin/env python3
"""Timing of the particle filter and of planning from particles on the GPU, HIP events after warm-up.

    python tools/gpu_particles_timing.py [--repeats 20] [--json out.json]

Reported (median us per call over `repeats` calls, each timed alone behind a sleep kernel so that the host's enqueue stays
out of the region):
  - ParticleBelief.update() of RockSample(7,8) at 4096 roots x 256 particles (2^20 particles), next to env.step() of a
    2^20-lane RockSample(7,8) batch — the filter steps 2^20 particles and then resamples them in the same launch;
  - the same update at 1024 roots x 1024 particles and 256 roots x 4096 (same particle count, more chunks per thread);
  - env.plan(belief=) next to env.plan() at bench.py's plan_rock15 shape: RockSample(15,15), 2048 roots, 1024 simulations
    per root, depth 64 (the belief: 256 particles per root, 4 simulations per particle).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda._sleep(2_000_000)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def update_us(gpa, roots, P, repeats):
    e = gpa.make("Rock-v0", batch_size=roots, seed=3, auto_reset=False, reuse_buffers=True)
    b = e.particle_belief(P)
    b.reset(e.reset())
    a = e.synthetic_actions()
    ob, rew, done, _ = e.step(a)
    ob, rew, done = ob.clone(), rew.clone(), done.clone()
    for _ in range(3):
        b.update(a, ob, rew, done)
    nm = b.n_match.clone()
    return timed(lambda: b.update(a, ob, rew, done), repeats), float((nm > 0).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import gym_pomdp_amd as gpa
    res = {"device": torch.cuda.get_device_name(0)}
    n = 1 << 20
    e = gpa.make("Rock-v0", batch_size=n, seed=3, reuse_buffers=True)
    e.reset()
    a = e.synthetic_actions()
    for _ in range(3):
        e.step(a)
    res["step_2e20_us"] = timed(lambda: e.step(a), args.repeats)
    for roots, P in ((4096, 256), (1024, 1024), (256, 4096)):
        us, frac = update_us(gpa, roots, P, args.repeats)
        res["update_%dx%d_us" % (roots, P)] = us
        res["update_%dx%d_roots_with_survivors" % (roots, P)] = frac
    res["update_over_step"] = res["update_4096x256_us"] / res["step_2e20_us"]
    roots, sims, depth, P = 2048, 1024, 64, 256
    pe = gpa.make("Rock-v0", board_size=15, num_rocks=15, batch_size=roots, seed=3, auto_reset=False, reuse_buffers=True)
    b = pe.particle_belief(P)
    b.reset(pe.reset())
    out_t = pe.plan(depth, sims_per_root=sims)
    out_b = pe.plan(depth, sims_per_root=sims, belief=b)
    res["plan_rock15_true_state_us"] = timed(lambda: pe.plan(depth, sims_per_root=sims, out=out_t), args.repeats)
    res["plan_rock15_belief_us"] = timed(lambda: pe.plan(depth, sims_per_root=sims, out=out_b, belief=b), args.repeats)
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
