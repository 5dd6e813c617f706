#!/usr/bin/env python
"""GPU box: plan(policy="preferred") against plan() in one process, HIP events after warm-up — the `plan_rock15` shape by
default (RockSample(15,15), 2048 roots x 1024 simulations, depth 64), from the true states and from 256 particles per root.
The roots are prepared by a few real heuristic-policy steps so that the policy has a history to read.  One JSON line
(profiles/r11_plan_preferred_timing.json).  Run it under `timeout`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--rocks", type=int, default=15)
    ap.add_argument("--roots", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--prep", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import gym_pomdp_amd as gpa
    e = gpa.make("Rock-v0", board_size=args.board, num_rocks=args.rocks, batch_size=args.roots, use_heuristic=True, auto_reset=False,
                 seed=1)
    ob = e.reset()
    hist = gpa.History(e)
    bel = e.particle_belief(args.particles)
    bel.reset(ob)
    for _ in range(args.prep):
        a, ob, _, _ = e.heuristic_steps(hist, 1)
        bel.update(a, ob)
    res = dict(tool="gpu_plan_preferred_timing", env="RockSample(%d,%d)" % (args.board, args.rocks), roots=args.roots, sims=args.sims,
               depth=args.depth, particles=args.particles, reps=args.reps,
               workspace_bytes=32 * args.rocks * args.roots * args.sims)
    for name, b in (("true", None), ("particles", bel)):
        outs = {}
        for policy in ("uniform", "preferred"):
            kw = dict(policy="preferred", history=hist) if policy == "preferred" else {}
            outs[policy] = e.plan(args.depth, args.sims, belief=b, **kw)
            fn = (lambda policy=policy, kw=kw: e.plan(args.depth, args.sims, belief=b, out=outs[policy], **kw))
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            med, best = timed(fn, args.reps)
            res["%s_%s_ms" % (name, policy)] = round(med, 4)
            res["%s_%s_min_ms" % (name, policy)] = round(best, 4)
        res["%s_ratio" % name] = round(res["%s_preferred_ms" % name] / res["%s_uniform_ms" % name], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
