#!/usr/bin/env python3
"""Timing of the stochastic controller loop (env.run_controller(StochasticController), pomdp_stoch_controller_episodes) against the
deterministic one (pomdp_controller_episodes) in the same run, HIP events around each call.

    python tools/gpu_stoch_controller_timing.py [--envs rock tag] [--lanes 1048576] [--steps 256] [--repeats 11] [--json out.json]

Workload: RockSample(7,8) and Tag, a fresh reset(), a seeded random 128-node controller with per-lane random start nodes, `steps`
steps in one call; every figure is the median over `repeats` runs from the same fresh batch, after a warm-up run.  Per env and sink
(packed records, returns statistics), microseconds per step of
  deterministic        env.run_controller(Controller): the loop without the draws;
  stoch_1x1            the same controller as a StochasticController (B = D = 1): the loop plus the lane's Philox block per step and
                       two candidate loops of no iterations — the same actions and successors as `deterministic`;
  stoch_<A>x1          B = n_actions candidates per node (random probabilities), D = 1: plus the action scan, A - 1 thresholds;
  stoch_<A>x4          B = n_actions, D = 4: plus the successor scan, 3 thresholds — on as many nodes as the 36 KB of tables hold
                       (Tag's 30 observations: 59 nodes; `nodes` of each entry says how many),
and each stochastic figure's ratio to `deterministic`.  Each env runs in a child process of its own under a time limit; the first
child that fails ends the run.  A sleep kernel in front of every timed region keeps the host's enqueue out of it."""
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
    import torch  # noqa: F401
    import gym_pomdp_amd as gpa
    from gym_pomdp_amd import _native
    from gym_pomdp_amd.stoch_controller import MAX_BYTES, footprint
    L = _native.lib()
    env_id, kw = ENV_IDS[args.env]
    n, k = args.lanes, args.steps
    e = gpa.make(env_id, batch_size=n, seed=args.seed, auto_reset=False, reuse_buffers=True, **kw)
    e.reset()
    st0, t1 = e._state.clone(), e.call_counter
    rng = np.random.RandomState(7)
    n_act, n_obs = e.action_space.n, e.observation_space.n
    start = rng.randint(0, NODES, n)
    det = gpa.Controller(e, rng.randint(0, n_act, NODES), rng.randint(0, NODES, (NODES, n_obs)), start=start)
    ctrls = {"deterministic": det, "stoch_1x1": gpa.StochasticController.from_controller(det)}
    for B, D in ((n_act, 1), (n_act, 4)):
        K = NODES
        while footprint(K, n_obs, B, D) > MAX_BYTES:
            K -= 1
        ap, nxp = rng.uniform(.05, 1.0, (K, B)), rng.uniform(.05, 1.0, (K, n_obs, D))
        ctrls["stoch_%dx%d" % (B, D)] = gpa.StochasticController(
            e, rng.randint(0, n_act, (K, B)), ap / ap.sum(-1, keepdims=True), rng.randint(0, K, (K, n_obs, D)),
            nxp / nxp.sum(-1, keepdims=True), start=start % K)

    def rewind(c):
        e._state.copy_(st0)
        e._done.zero_()
        e.call_counter = t1
        c.reset_nodes()

    res = {"env": args.env, "lanes": n, "steps": k, "repeats": args.repeats, "kernels": {}, "nodes": {}, "table_bytes": {},
           "live_frac_at_end": {}}
    packed, stats = e.trajectory_buffers(k, "packed"), gpa.EpisodeStats(e)
    for name, c in ctrls.items():
        res["nodes"][name] = c.n_nodes
        res["table_bytes"][name] = (footprint(c.n_nodes, n_obs, c.n_act_cand, c.n_next_cand) if name != "deterministic"
                                    else (2 * c.n_nodes * n_obs + c.n_nodes + 15) // 16 * 16)
        for sink, kwargs in (("packed", dict(out=packed)), ("returns", dict(stats=stats))):
            def fn(c=c, kwargs=kwargs):
                rewind(c)
                stats.reset()
                return lambda: e.run_controller(c, k, **kwargs)
            res["%s_%s_us_per_step" % (name, sink)] = timed(fn, args.repeats) * 1e3 / k
            res["kernels"]["%s_%s" % (name, sink)] = L.pomdp_last_fused_kernel().decode()
        res["live_frac_at_end"][name] = round(1.0 - float(e._done.float().mean().item()), 4)
    for name in ctrls:
        if name != "deterministic":
            for sink in ("packed", "returns"):
                res["%s_to_deterministic_%s" % (name, sink)] = (res["%s_%s_us_per_step" % (name, sink)]
                                                                / res["deterministic_%s_us_per_step" % sink])
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
            sys.exit("gpu_stoch_controller_timing: %s ended with status %d" % (env, p.returncode))
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"tool": "tools/gpu_stoch_controller_timing.py", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
