#!/usr/bin/env python3
"""Timing of the frozen-lane loops (env.finish_episodes, pomdp_finish_episodes) on the GPU, HIP events around each call.

    python tools/episodes_timing.py [--env rock] [--lanes 1048576] [--steps 256] [--repeats 5] [--json out.json]

Workload: RockSample(7,8) by default, a fresh reset(), the synthetic policy, `steps` steps; every figure is the median over
`repeats` runs from the same fresh batch.  Reported:
  - us per step of finish_episodes in the returns and packed sinks against the auto-reset fused launches over the same k
    (collect_returns / collect_synthetic(layout="packed")): the same policy, the same lanes, lanes that never freeze;
  - the whole finish_episodes call against a Python loop of `steps` x (synthetic_actions() + step()) with auto_reset=False —
    what a frozen-mode caller had before;
  - how the time per step falls as the episodes end: single launches of 16, 32, .. steps from the fresh batch; the difference
    between two lengths per step (the launch's fixed part cancels) next to the fraction of lanes still live at the shorter one.
A sleep kernel in front of every timed region keeps the host's enqueue out of it.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

ENV_IDS = {"rock": ("Rock-v0", {}), "rock15": ("Rock-v0", dict(board_size=15, num_rocks=15)), "stochrock": ("StochasticRock-v0", {}),
           "tag": ("Tag-v0", {}), "tiger": ("Tiger-v0", {}), "network": ("Network-v0", {}), "battleship": ("Battleship-v0", {})}


def timed(fn, repeats):
    """median milliseconds between two HIP events around the callable fn() returns (fn itself — building a fresh batch — is
    not timed).  A sleep kernel runs in front of the first event, so the region holds the GPU work and not the host's enqueue."""
    ts = []
    for _ in range(repeats):
        run = fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda._sleep(2_000_000)
        a.record()
        run()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="rock", choices=sorted(ENV_IDS))
    ap.add_argument("--lanes", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import gym_pomdp_amd as gpa
    from gym_pomdp_amd import _native
    L = _native.lib()
    env_id, kw = ENV_IDS[args.env]
    n, k = args.lanes, args.steps

    def fresh(auto_reset, **extra):
        e = gpa.make(env_id, batch_size=n, seed=args.seed, auto_reset=auto_reset, reuse_buffers=True, **kw, **extra)
        e.reset()
        return e

    res = {"env": args.env, "lanes": n, "steps": k, "repeats": args.repeats}
    # the frozen loops and the auto-reset loops over the same k steps
    runs = {
        "finish_returns": lambda: (lambda e: (lambda: e.finish_episodes(k)))(fresh(False)),
        "finish_packed": lambda: (lambda e, out: (lambda: e.finish_episodes(k, layout="packed", out=out)))(
            *(lambda e: (e, e.trajectory_buffers(k, "packed")))(fresh(False))),
        "auto_returns": lambda: (lambda e: (lambda: e.collect_returns(k)))(fresh(True)),
        "auto_packed": lambda: (lambda e, out: (lambda: e.collect_synthetic(k, out=out)))(
            *(lambda e: (e, e.trajectory_buffers(k, "packed")))(fresh(True))),
    }
    kernels = {}
    for name, make in runs.items():
        ms = timed(make, args.repeats)
        kernels[name] = L.pomdp_last_fused_kernel().decode()
        res[name + "_us_per_step"] = ms * 1e3 / k
    res["kernels"] = kernels
    res["returns_ratio_to_auto_reset"] = res["finish_returns_us_per_step"] / res["auto_returns_us_per_step"]
    res["packed_ratio_to_auto_reset"] = res["finish_packed_us_per_step"] / res["auto_packed_us_per_step"]

    # a Python loop over step() with auto_reset=False (the synthetic policy's actions from its own launch each step)
    def python_loop():
        e = fresh(False)

        def run():
            for _ in range(k):
                e.step(e.synthetic_actions())
        return run
    res["python_loop_ms"] = timed(python_loop, max(1, args.repeats // 2))
    res["finish_returns_ms"] = res["finish_returns_us_per_step"] * k * 1e-3
    res["speedup_vs_python_loop"] = res["python_loop_ms"] / res["finish_returns_ms"]

    # us per step as the episodes end: single launches of k = 16 .. steps steps from the fresh batch; the time between two
    # lengths, per step, is what those steps cost (the launch's fixed part cancels), next to the lanes still live there
    ks = [c for c in (16, 32, 64, 128, 256) if c <= k]
    by_k = {}
    for c in ks:
        e = fresh(False)
        ms = {"finish_returns": timed(lambda: (lambda e: (lambda: e.finish_episodes(c)))(fresh(False)), args.repeats),
              "auto_returns": timed(lambda: (lambda e: (lambda: e.collect_returns(c)))(fresh(True)), args.repeats)}
        e.finish_episodes(c)
        by_k[c] = dict(ms, live_frac=round(1.0 - float(e._done.float().mean().item()), 4))
    marg = []
    for c0, c1 in zip(ks[:-1], ks[1:]):
        marg.append({"steps": [c0, c1], "live_frac_at_start": by_k[c0]["live_frac"],
                     "finish_returns_us_per_step": (by_k[c1]["finish_returns"] - by_k[c0]["finish_returns"]) * 1e3 / (c1 - c0),
                     "auto_returns_us_per_step": (by_k[c1]["auto_returns"] - by_k[c0]["auto_returns"]) * 1e3 / (c1 - c0)})
    res["launch_ms_by_steps"] = {str(c): v for c, v in by_k.items()}
    res["marginal"] = marg
    res["first16_ratio_to_auto_reset"] = by_k[ks[0]]["finish_returns"] / by_k[ks[0]]["auto_returns"] if ks else None
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
