#!/usr/bin/env python
"""GPU box: search() against plan() at an equal simulation budget in one process, HIP events after warm-up — BASELINE.json
configs[4]'s shape by default: RockSample(15,15), 2048 roots, search with 16 trees per root x 64 simulations of depth 64
against plan(64, 1024), both 1024 simulations per root, from the true states and from 256 particles per root.  The roots
are a few real steps into their episodes.  One JSON line (profiles/r24_tree_search_timing.json), with the search kernel's
resources (tools/kernel_resources.py; compiled on the spot, no GPU work).  Run it under `timeout`.
--preferred: the preferred-policy arm instead (profiles/r25_tree_search_timing.json) — an env with use_heuristic=True whose
roots are `--prep` heuristic-policy steps into their episodes; search(policy="preferred", history=) without priors and with
(--prior-n, --prior-v), and the uniform search() on the same roots in the same run, from the true states and from particles."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


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
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--rocks", type=int, default=15)
    ap.add_argument("--roots", type=int, default=2048)
    ap.add_argument("--trees", type=int, default=16)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--ucb-c", type=float, default=20.0)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--prep", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--preferred", action="store_true")
    ap.add_argument("--prior-n", type=int, default=3)
    ap.add_argument("--prior-v", type=float, default=5.0)
    args = ap.parse_args()
    import gym_pomdp_amd as gpa
    if args.preferred:
        return preferred_arm(args, gpa)
    e = gpa.make("Rock-v0", board_size=args.board, num_rocks=args.rocks, batch_size=args.roots, auto_reset=False, seed=1)
    ob = e.reset()
    bel = e.particle_belief(args.particles)
    bel.reset(ob)
    for _ in range(args.prep):
        a = e.synthetic_actions()
        ob, rew, done, _ = e.step(a)
        bel.update(a, ob)
    budget = args.trees * args.sims
    res = dict(tool="gpu_tree_search_timing", env="RockSample(%d,%d)" % (args.board, args.rocks), roots=args.roots,
               trees_per_root=args.trees, sims_per_tree=args.sims, depth=args.depth, ucb_c=args.ucb_c, particles=args.particles,
               sims_per_root=budget, reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    for name, b in (("true", None), ("particles", bel)):
        s_out = e.search(args.depth, args.sims, args.trees, args.ucb_c, belief=b, diagnostics=True)
        p_out = e.plan(args.depth, budget, belief=b)
        search = lambda: e.search(args.depth, args.sims, args.trees, args.ucb_c, belief=b, out=s_out, diagnostics=True)
        plan = lambda: e.plan(args.depth, budget, belief=b, out=p_out)
        for what, fn in (("search", search), ("plan", plan)):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            med, lo, hi = timed(fn, args.reps)
            res["%s_%s_ms" % (name, what)] = round(med, 4)
            res["%s_%s_min_ms" % (name, what)] = round(lo, 4)
            res["%s_%s_max_ms" % (name, what)] = round(hi, 4)
        res["%s_ratio" % name] = round(res["%s_search_ms" % name] / res["%s_plan_ms" % name], 3)
        steps = int(s_out["sim_steps"].sum().item())
        res["%s_search_sim_steps" % name] = steps
        res["%s_search_tree_steps" % name] = int(s_out["sim_tree_steps"].sum().item())
        res["%s_search_steps_per_s" % name] = round(steps / (res["%s_search_ms" % name] * 1e-3), 1)
        res["%s_search_mean_nodes" % name] = round(float(s_out["n_nodes"].double().mean().item()), 2)
        res["%s_best_agree" % name] = round(float((s_out["best"] == p_out["best"]).double().mean().item()), 4)
    res["workspace_bytes"] = int(s_out["_workspace"].numel() * 8)
    if not args.no_resources:
        import kernel_resources as kr
        want = "tree_search_kernel<RockEnv<%d, false> >" % (1 if args.rocks <= 12 else 2)
        res["resources"] = [r for r in kr.collect(units=["tree_search.hip"]) if r["kernel"] in (want, "tree_merge_kernel")]
    print(json.dumps(res))


def preferred_arm(args, gpa):
    e = gpa.make("Rock-v0", board_size=args.board, num_rocks=args.rocks, batch_size=args.roots, auto_reset=False, seed=1,
                 use_heuristic=True)
    ob = e.reset()
    hist = gpa.History(e)
    bel = e.particle_belief(args.particles)
    bel.reset(ob)
    for _ in range(args.prep):
        a, ob, rew, done = e.heuristic_steps(hist, 1)
        bel.update(a, ob)
    res = dict(tool="gpu_tree_search_timing --preferred", env="RockSample(%d,%d)" % (args.board, args.rocks), roots=args.roots,
               trees_per_root=args.trees, sims_per_tree=args.sims, depth=args.depth, ucb_c=args.ucb_c, particles=args.particles,
               sims_per_root=args.trees * args.sims, prep_heuristic_steps=args.prep, prior_n=args.prior_n, prior_v=args.prior_v,
               reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    arms = (("uniform", {}), ("preferred", dict(policy="preferred", history=hist)),
            ("preferred_priors", dict(policy="preferred", history=hist, prior_n=args.prior_n, prior_v=args.prior_v)))
    for name, b in (("true", None), ("particles", bel)):
        for what, kw in arms:
            out = e.search(args.depth, args.sims, args.trees, args.ucb_c, belief=b, diagnostics=True, **kw)
            fn = lambda: e.search(args.depth, args.sims, args.trees, args.ucb_c, belief=b, out=out, diagnostics=True, **kw)
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            med, lo, hi = timed(fn, args.reps)
            key = "%s_%s" % (name, what)
            res[key + "_ms"], res[key + "_min_ms"], res[key + "_max_ms"] = round(med, 4), round(lo, 4), round(hi, 4)
            steps = int(out["sim_steps"].sum().item())
            res[key + "_sim_steps"] = steps
            res[key + "_tree_steps"] = int(out["sim_tree_steps"].sum().item())
            res[key + "_steps_per_s"] = round(steps / (med * 1e-3), 1)
            res[key + "_mean_nodes"] = round(float(out["n_nodes"].double().mean().item()), 2)
            if "_policy_workspace" in out:
                res["policy_workspace_bytes"] = int(out["_policy_workspace"].numel() * 8)
            res["workspace_bytes"] = int(out["_workspace"].numel() * 8)
        for what in ("preferred", "preferred_priors"):
            res["%s_%s_over_uniform" % (name, what)] = round(res["%s_%s_ms" % (name, what)] / res["%s_uniform_ms" % name], 3)
    if not args.no_resources:
        import kernel_resources as kr
        v = 1 if args.rocks <= 12 else 2
        res["resources"] = [r for r in kr.collect(units=["tree_search_preferred.hip"]) if r["kernel"] == "tree_preferred_kernel<RockEnv<%d, false> >" % v] + \
                           [r for r in kr.collect(units=["tree_search.hip"]) if r["kernel"] == "tree_search_kernel<RockEnv<%d, false> >" % v]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
