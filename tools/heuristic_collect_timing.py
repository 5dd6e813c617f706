#!/usr/bin/env python
"""GPU box: what keeping every step of the heuristic-policy loop costs, in one process, HIP events after warm-up.
RockSample(7,8), RockSample(15,15) and Tag at 2^20 lanes; 128 untimed heuristic steps after reset() put the policy in its
steady state, then 256-step launches.  Four arms, taken in turn within each of the --reps rounds (median and min per arm):
    a  heuristic_steps(h, 256)                       nothing kept per step
    b  collect_heuristic(h, 256, layout="packed")    one 4-byte record per lane-step
    c  collect_heuristic(h, 256, layout="narrow")    four typed planes per step
    d  256 x heuristic_steps(h, 1), each followed by copying the four outputs into preallocated rows: what a caller who wants
       every step had before collect_heuristic
On a tree without collect_heuristic (an older revision, for a same-box A/B) arms b and c are skipped.  One JSON line
(profiles/r18_heuristic_collect_timing.json collects them).  Run it under `timeout`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENVS = {"rock": ("Rock-v0", dict(use_heuristic=True)), "rock15": ("Rock-v0", dict(board_size=15, num_rocks=15, use_heuristic=True)),
        "tag": ("Tag-v0", {})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="rock,rock15,tag")
    ap.add_argument("--lanes", type=int, default=1 << 20)
    ap.add_argument("--prep", type=int, default=128)
    ap.add_argument("--launch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import gym_pomdp_amd as gpa
    n, k = args.lanes, args.launch
    res = dict(tool="heuristic_collect_timing", label=args.label, lanes=n, steps_per_launch=k, prep_steps=args.prep, reps=args.reps,
               unit="us per step", envs={})
    for name in args.envs.split(","):
        env_id, kw = ENVS[name]
        e = gpa.make(env_id, batch_size=n, seed=1, lane_offset=1 << 21, reuse_buffers=True, **kw)
        e.reset()
        h = gpa.History(e)
        e.heuristic_steps(h, args.prep)
        rows = e.trajectory_buffers(k)                                   # arm d: the four columns a caller keeps
        arms = {"a": lambda: e.heuristic_steps(h, k)}
        if hasattr(e, "collect_heuristic"):
            out = {lay: e.trajectory_buffers(k, lay) for lay in ("packed", "narrow")}
            arms["b"] = lambda: e.collect_heuristic(h, k, layout="packed", out=out["packed"])
            arms["c"] = lambda: e.collect_heuristic(h, k, layout="narrow", out=out["narrow"])

        def per_step():
            for s in range(k):
                a, o, r, d = e.heuristic_steps(h, 1)
                rows["action"][s].copy_(a); rows["ob"][s].copy_(o); rows["reward"][s].copy_(r); rows["done"][s].copy_(d)
        arms["d"] = per_step
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        ms = {arm: [] for arm in arms}
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.reps):
            for arm, fn in arms.items():
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                ms[arm].append(t0.elapsed_time(t1))
        r = {}
        for arm, v in ms.items():
            v.sort()
            r[arm] = dict(median=round(1e3 * v[len(v) // 2] / k, 4), min=round(1e3 * v[0] / k, 4), max=round(1e3 * v[-1] / k, 4))
        res["envs"][name] = r
        del e, h, rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
