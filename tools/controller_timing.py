#!/usr/bin/env python3
"""Timing of the controller loop (env.run_controller, pomdp_controller_episodes) on the GPU, HIP events around each call.

    python tools/controller_timing.py [--envs rock tag] [--lanes 1048576] [--steps 256] [--repeats 11] [--json out.json]

Workload: RockSample(7,8) and Tag, a fresh reset(), a seeded random 128-node controller with per-lane random start nodes,
`steps` steps in one call; every figure is the median over `repeats` runs from the same fresh batch, after a warm-up run.
Per env and sink (packed records, returns statistics), microseconds per step of
  (a) controller      env.run_controller;
  (b) tape            env.finish_episodes(actions=tape) on the action bytes run (a) recorded — the loop the launcher picks
                      for such a caller (RockSample at 2^20 lanes: the quad-per-thread one) — and tape_general, the same
                      tape at an odd address, which the launcher sends to the general one-lane-per-thread loop: the same loop
                      as (a) with a global tape read in place of two LDS reads;
  (c) python_loop     a Python loop over step() with the controller evaluated in torch between the steps — what a caller with
                      a closed-loop policy had before (one figure per env: it has no sink).
Each env runs in a child process of its own under a time limit; the first child that fails ends the run.
A sleep kernel in front of every timed region keeps the host's enqueue out of it."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ENV_IDS = {"rock": ("Rock-v0", {}), "stochrock": ("StochasticRock-v0", {}), "tag": ("Tag-v0", {}), "tiger": ("Tiger-v0", {}),
           "network": ("Network-v0", {}), "battleship": ("Battleship-v0", {})}
NODES = 128


def timed(fn, repeats):
    """median milliseconds between two HIP events around the callable fn() returns (fn itself — putting the fresh batch back —
    is not timed), after one untimed run"""
    import torch
    ts = []
    for i in range(repeats + 1):
        run = fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda._sleep(2_000_000)
        a.record()
        run()
        b.record()
        b.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def one_env(args):
    import numpy as np
    import torch
    import gym_pomdp_amd as gpa
    from gym_pomdp_amd import _native
    L = _native.lib()
    env_id, kw = ENV_IDS[args.env]
    n, k = args.lanes, args.steps
    e = gpa.make(env_id, batch_size=n, seed=args.seed, auto_reset=False, reuse_buffers=True, **kw)
    e.reset()
    st0, t1 = e._state.clone(), e.call_counter
    rng = np.random.RandomState(7)
    n_act, n_obs = e.action_space.n, e.observation_space.n
    ctrl = gpa.Controller(e, rng.randint(0, n_act, NODES), rng.randint(0, NODES, (NODES, n_obs)), start=rng.randint(0, NODES, n))

    def rewind():
        e._state.copy_(st0)
        e._done.zero_()
        e.call_counter = t1
        ctrl.reset_nodes()

    res = {"env": args.env, "lanes": n, "steps": k, "repeats": args.repeats, "nodes": NODES, "kernels": {}}
    rewind()
    narrow = e.run_controller(ctrl, k, layout="narrow")
    res["live_frac_at_end"] = round(1.0 - float(e._done.float().mean().item()), 4)
    tape = narrow["traj"][:k, 0, :n]                                   # the recorded action bytes, a tape as they stand
    odd = torch.zeros(k * (n + 4) + 1, dtype=torch.uint8, device=e.device)[1:].view(k, n + 4)[:, :n]
    odd.copy_(tape)                                                   # the same rows from an odd address
    packed, stats = e.trajectory_buffers(k, "packed"), gpa.EpisodeStats(e)

    for sink, kwargs in (("packed", dict(out=packed)), ("returns", dict(stats=stats))):
        runs = {"controller": lambda: e.run_controller(ctrl, k, **kwargs),
                "tape": lambda: e.finish_episodes(k, actions=tape, **kwargs),
                "tape_general": lambda: e.finish_episodes(k, actions=odd, **kwargs)}
        for name, call in runs.items():
            def fn(call=call):
                rewind()
                stats.reset()
                return call
            res["%s_%s_us_per_step" % (name, sink)] = timed(fn, args.repeats) * 1e3 / k
            res["kernels"]["%s_%s" % (name, sink)] = L.pomdp_last_fused_kernel().decode()
        res["controller_to_tape_%s" % sink] = res["controller_%s_us_per_step" % sink] / res["tape_%s_us_per_step" % sink]
        res["controller_to_tape_general_%s" % sink] = res["controller_%s_us_per_step" % sink] / res["tape_general_%s_us_per_step" % sink]

    act, nxt = ctrl.action, ctrl.next.long()

    def python_loop():
        rewind()
        node = ctrl.node.long()

        def run():
            q = node
            for _ in range(k):
                ob, _, done, _ = e.step(act[q])
                q = torch.where(done, q, nxt[q, ob.long()])            # a frozen lane reports ob 0: its node stays
        return run
    res["python_loop_us_per_step"] = timed(python_loop, max(3, args.repeats // 2)) * 1e3 / k
    for sink in ("packed", "returns"):
        res["python_loop_to_controller_%s" % sink] = res["python_loop_us_per_step"] / res["controller_%s_us_per_step" % sink]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", nargs="+", default=["rock", "tag"], choices=sorted(ENV_IDS))
    ap.add_argument("--env", default=None, help=argparse.SUPPRESS)     # the child's: one env in this process
    ap.add_argument("--lanes", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.env:
        return one_env(args)
    results = []
    for env in args.envs:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--env", env, "--lanes", str(args.lanes),
               "--steps", str(args.steps), "--repeats", str(args.repeats), "--seed", str(args.seed)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:                                          # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit("controller_timing: %s ended with status %d" % (env, p.returncode))
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"tool": "tools/controller_timing.py", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
