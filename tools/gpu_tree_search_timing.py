#!/usr/bin/env python
"""GPU box: search() against plan() at an equal simulation budget in one process, HIP events after warm-up — BASELINE.json
configs[4]'s shape by default: RockSample(15,15), 2048 roots, search with 16 trees per root x 64 simulations of depth 64
against plan(64, 1024), both 1024 simulations per root, from the true states and from 256 particles per root.  The roots
are a few real steps into their episodes.  One JSON line (profiles/r24_tree_search_timing.json), with the search kernel's
resources (tools/kernel_resources.py; compiled on the spot, no GPU work).  Run it under `timeout`.
--preferred: the preferred-policy arm instead (profiles/r25_tree_search_timing.json) — an env with use_heuristic=True whose
roots are `--prep` heuristic-policy steps into their episodes; search(policy="preferred", history=) without priors and with
(--prior-n, --prior-v), and the uniform search() on the same roots in the same run, from the true states and from particles.
--keep: the kept-tree arm instead (profiles/r26_tree_keep_timing.json), from the true states and from particles: search() — the
yardstick, its kernel untouched —, search(tree=) from empty trees, search(tree=) on the `--keep-step`-th consecutive
search_step(tree=) of the same roots, and tree.advance() alone, with the nodes kept and held there; then `--episodes` Tag
episodes of at most `--episode-steps` steps played by search_step() with and without tree= at the same budget: the mean
discounted return of each (recorded, not judged).
--keep --preferred: the kept-tree arm of the preferred-policy search (profiles/r27_tree_keep_preferred_timing.json) on the
--preferred arm's roots, `--capacity` nodes per tree (default 2 * sims + 1), without priors and with (--prior-n, --prior-v), from
the true states and from particles: search(policy="preferred") — the yardstick, its kernel untouched —, search(tree=) from
empty preferred trees, the search of the `--keep-step`-th consecutive search_step(tree=) with the nodes kept there and the
share of in-tree steps, and tree.advance() alone; then the Tag episodes as above under policy="preferred" with the priors."""
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
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--capacity", type=int, default=None, help="nodes per kept tree (default 2 * sims + 1)")
    ap.add_argument("--keep-step", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--episode-steps", type=int, default=90)
    args = ap.parse_args()
    import gym_pomdp_amd as gpa
    if args.keep and args.preferred:
        return keep_preferred_arm(args, gpa)
    if args.preferred:
        return preferred_arm(args, gpa)
    if args.keep:
        return keep_arm(args, gpa)
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


def stats(ms):
    ms = sorted(ms)
    return round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)


def keep_arm(args, gpa):
    D, S, W, c = args.depth, args.sims, args.trees, args.ucb_c
    Cn = 2 * S + 1 if args.capacity is None else args.capacity
    e = gpa.make("Rock-v0", board_size=args.board, num_rocks=args.rocks, batch_size=args.roots, auto_reset=False, seed=1)
    ob = e.reset()
    bel = e.particle_belief(args.particles)
    bel.reset(ob)
    for _ in range(args.prep):
        a = e.synthetic_actions()
        ob, rew, done, _ = e.step(a)
        bel.update(a, ob)
    res = dict(tool="gpu_tree_search_timing --keep", env="RockSample(%d,%d)" % (args.board, args.rocks), roots=args.roots,
               trees_per_root=W, sims_per_tree=S, depth=D, ucb_c=c, particles=args.particles, node_capacity=Cn,
               keep_step=args.keep_step, reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0))
    state0, t0, done0 = e.state.clone(), e.call_counter, e.done.clone()
    parts0, tb0 = bel.particles.clone(), bel.call_counter
    tree = e.search_tree(W, Cn, D)
    res["keep_workspace_bytes"] = 2 * tree._bytes
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def restore():
        e.set_state(state0)
        e._done.copy_(done0)
        e.call_counter = t0
        bel.set_particles(parts0)
        bel.call_counter = tb0
        tree.clear()

    for name, b in (("true", None), ("particles", bel)):
        restore()
        s_out = e.search(D, S, W, c, belief=b)
        e.call_counter = t0
        k_out = e.search(D, S, W, c, belief=b, tree=tree)
        res["%s_empty_equals_search" % name] = bool(all(torch.equal(s_out[k], k_out[k]) for k in ("q", "visits", "best", "value")))
        # arm 1: search(), the parent's kernel; arm 2: the resumed search from empty trees (cleared outside the timed span)
        for what, fn, before in (("search", lambda: e.search(D, S, W, c, belief=b, out=s_out), lambda: None),
                                 ("resume_empty", lambda: e.search(D, S, W, c, belief=b, out=k_out, tree=tree), tree.clear)):
            ms = []
            for i in range(args.warmup + args.reps):
                e.call_counter = t0
                before()
                x, y = ev(), ev()
                x.record()
                fn()
                y.record()
                y.synchronize()
                if i >= args.warmup:
                    ms.append(x.elapsed_time(y))
            res["%s_%s_ms" % (name, what)], res["%s_%s_min_ms" % (name, what)], res["%s_%s_max_ms" % (name, what)] = stats(ms)
        lo, hi, med = res["%s_search_min_ms" % name], res["%s_search_max_ms" % name], res["%s_resume_empty_ms" % name]
        res["%s_resume_empty_over_search" % name] = round(med / res["%s_search_ms" % name], 4)
        res["%s_resume_empty_inside_search_spread" % name] = bool(lo <= med <= hi)
        # arm 3: the search of the keep_step-th consecutive search_step(tree=); arm 4: its advance alone
        ms_s, ms_a, kept, held, live = [], [], [], [], []
        for i in range(args.warmup + args.reps):
            restore()
            for _ in range(args.keep_step - 1):
                e.search_step(D, S, W, c, belief=b, out=k_out, tree=tree)
            kept.append(float(tree.n_nodes.double().mean().item()))
            live.append(float((tree.n_nodes > 0).double().mean().item()))
            x, y, z, w = ev(), ev(), ev(), ev()
            x.record()
            p = e.search(D, S, W, c, belief=b, out=k_out, tree=tree)
            y.record()
            o2, r2, d2, _ = e.step(p["best"])
            z.record()
            tree.advance(p["best"], o2, drop=d2)
            w.record()
            w.synchronize()
            held.append(float(p["n_nodes"].double().mean().item()))
            if i >= args.warmup:
                ms_s.append(x.elapsed_time(y))
                ms_a.append(z.elapsed_time(w))
        res["%s_resume_kept_ms" % name], res["%s_resume_kept_min_ms" % name], res["%s_resume_kept_max_ms" % name] = stats(ms_s)
        res["%s_advance_ms" % name], res["%s_advance_min_ms" % name], res["%s_advance_max_ms" % name] = stats(ms_a)
        res["%s_mean_kept_nodes" % name] = round(kept[-1], 3)                 # per tree, before the timed search (empty trees count 0)
        res["%s_trees_with_kept_nodes" % name] = round(live[-1], 4)
        res["%s_mean_nodes_after" % name] = round(held[-1], 3)
        res["%s_lanes_done" % name] = round(float(e.done.double().mean().item()), 4)
    # whether reuse changes the decisions: Tag episodes from the true states, with and without tree=, the same seeds
    for name, use in (("tag_without_tree", False), ("tag_with_tree", True)):
        t = gpa.make("Tag-v0", batch_size=args.episodes, auto_reset=False, seed=1)
        t.reset()
        tr = t.search_tree(W, Cn, D) if use else None
        ret = torch.zeros(args.episodes, dtype=torch.float64, device=t.device)
        disc, out = 1.0, None
        for _ in range(args.episode_steps):
            if use and W * (tr.searches + 1) * S > 0x7FFFFFFF:
                tr.clear()
            kw = dict(tree=tr) if use else {}
            o2, r2, d2, _, out = t.search_step(D, S, W, 10.0, out=out, **kw)
            ret += disc * r2.double()                                         # a frozen lane's reward is 0
            disc *= t._discount
        res[name + "_mean_return"] = round(float(ret.mean().item()), 4)
        res[name + "_return_stderr"] = round(float(ret.std().item()) / args.episodes ** .5, 4)
        res[name + "_episodes_ended"] = round(float(t.done.double().mean().item()), 4)
    res.update(tag_episodes=args.episodes, tag_episode_steps=args.episode_steps, tag_ucb_c=10.0)
    if not args.no_resources:
        import kernel_resources as kr
        v = 1 if args.rocks <= 12 else 2
        res["resources"] = [r for r in kr.collect(units=["tree_keep.hip"]) if r["kernel"] in ("tree_resume_kernel<RockEnv<%d, false> >" % v, "tree_advance_kernel")] + \
                           [r for r in kr.collect(units=["tree_search.hip"]) if r["kernel"] == "tree_search_kernel<RockEnv<%d, false> >" % v]
    print(json.dumps(res))


def keep_preferred_arm(args, gpa):
    D, S, W, c = args.depth, args.sims, args.trees, args.ucb_c
    Cn = 2 * S + 1 if args.capacity is None else args.capacity
    res = dict(tool="gpu_tree_search_timing --keep --preferred", env="RockSample(%d,%d)" % (args.board, args.rocks), roots=args.roots,
               trees_per_root=W, sims_per_tree=S, depth=D, ucb_c=c, particles=args.particles, node_capacity=Cn,
               prep_heuristic_steps=args.prep, keep_step=args.keep_step, prior_v=args.prior_v, reps=args.reps, warmup=args.warmup,
               device=torch.cuda.get_device_name(0))
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def roots():
        """the --preferred arm's roots, built anew: search_step() moves the env, its History and its side statistics"""
        e = gpa.make("Rock-v0", board_size=args.board, num_rocks=args.rocks, batch_size=args.roots, auto_reset=False, seed=1,
                     use_heuristic=True)
        ob = e.reset()
        hist = gpa.History(e)
        bel = e.particle_belief(args.particles)
        bel.reset(ob)
        for _ in range(args.prep):
            a, ob, rew, done = e.heuristic_steps(hist, 1)
            bel.update(a, ob)
        return e, hist, bel

    for pn in (0, args.prior_n):
        pkw = dict(policy="preferred", prior_n=pn, prior_v=args.prior_v if pn else 0.0)
        for src in ("true", "particles"):
            name = "%s_n%d" % (src, pn)
            e, hist, bel = roots()
            b = bel if src == "particles" else None
            t0 = e.call_counter
            tree = e.search_tree(W, Cn, D, **pkw)
            res["keep_workspace_bytes"] = 2 * tree._bytes
            s_out = e.search(D, S, W, c, belief=b, history=hist, **pkw)
            e.call_counter = t0
            k_out = e.search(D, S, W, c, belief=b, history=hist, policy="preferred", tree=tree)
            res[name + "_empty_equals_search"] = bool(all(torch.equal(s_out[k], k_out[k]) for k in ("q", "visits", "best", "value")))
            # arm 1: search(policy="preferred"), the parent's kernel; arm 2: resumed from empty trees (cleared outside the timed span)
            for what, fn, before in (("search", lambda: e.search(D, S, W, c, belief=b, out=s_out, history=hist, **pkw), lambda: None),
                                     ("resume_empty", lambda: e.search(D, S, W, c, belief=b, out=k_out, history=hist, policy="preferred",
                                                                       tree=tree), tree.clear)):
                ms = []
                for i in range(args.warmup + args.reps):
                    e.call_counter = t0
                    before()
                    x, y = ev(), ev()
                    x.record()
                    fn()
                    y.record()
                    y.synchronize()
                    if i >= args.warmup:
                        ms.append(x.elapsed_time(y))
                res[name + "_%s_ms" % what], res[name + "_%s_min_ms" % what], res[name + "_%s_max_ms" % what] = stats(ms)
            lo, hi, med = res[name + "_search_min_ms"], res[name + "_search_max_ms"], res[name + "_resume_empty_ms"]
            res[name + "_resume_empty_over_search"] = round(med / res[name + "_search_ms"], 4)
            res[name + "_resume_empty_inside_search_spread"] = bool(lo <= med <= hi)
            # arm 3: the search of the keep_step-th consecutive search_step(tree=); arm 4: its advance alone
            ms_s, ms_a = [], []
            for i in range(args.warmup + args.reps):
                e, hist, bel = roots()
                b = bel if src == "particles" else None
                tree = e.search_tree(W, Cn, D, **pkw)
                out = None
                for _ in range(args.keep_step - 1):                          # diagnostics on: `out` holds every buffer the timed search writes
                    out = e.search_step(D, S, W, c, belief=b, out=out, history=hist, policy="preferred", tree=tree, diagnostics=True)[4]
                kept = tree.n_nodes.clone()
                x, y, z, w = ev(), ev(), ev(), ev()
                x.record()
                p = e.search(D, S, W, c, belief=b, out=out, history=hist, policy="preferred", tree=tree, diagnostics=True)
                y.record()
                o2, r2, d2, _ = e.step(p["best"])
                z.record()
                tree.advance(p["best"], o2, drop=d2)
                w.record()
                w.synchronize()
                if i >= args.warmup:
                    ms_s.append(x.elapsed_time(y))
                    ms_a.append(z.elapsed_time(w))
            res[name + "_resume_kept_ms"], res[name + "_resume_kept_min_ms"], res[name + "_resume_kept_max_ms"] = stats(ms_s)
            res[name + "_advance_ms"], res[name + "_advance_min_ms"], res[name + "_advance_max_ms"] = stats(ms_a)
            res[name + "_resume_kept_over_search"] = round(res[name + "_resume_kept_ms"] / res[name + "_search_ms"], 4)
            res[name + "_mean_kept_nodes"] = round(float(kept.double().mean().item()), 3)     # per tree, before the timed search
            res[name + "_max_kept_nodes"] = int(kept.max().item())
            res[name + "_trees_with_kept_nodes"] = round(float((kept > 0).double().mean().item()), 4)
            res[name + "_mean_nodes_after"] = round(float(p["n_nodes"].double().mean().item()), 3)
            res[name + "_tree_step_share"] = round(float(p["sim_tree_steps"].sum().item()) / max(float(p["sim_steps"].sum().item()), 1.0), 4)
            res[name + "_lanes_done"] = round(float(e.done.double().mean().item()), 4)
    # whether reuse changes the decisions: Tag episodes from the true states under the preferred policy with priors
    for name, use in (("tag_without_tree", False), ("tag_with_tree", True)):
        t = gpa.make("Tag-v0", batch_size=args.episodes, auto_reset=False, seed=1)
        t.reset()
        th = gpa.History(t)
        tr = t.search_tree(W, Cn, D, policy="preferred", prior_n=args.prior_n, prior_v=args.prior_v) if use else None
        ret = torch.zeros(args.episodes, dtype=torch.float64, device=t.device)
        disc, out = 1.0, None
        for _ in range(args.episode_steps):
            if use and W * ((tr.searches + 1) * S + 5 * args.prior_n) > 0x7FFFFFFF:
                tr.clear()
            kw = dict(tree=tr) if use else dict(prior_n=args.prior_n, prior_v=args.prior_v)
            o2, r2, d2, _, out = t.search_step(D, S, W, 10.0, out=out, policy="preferred", history=th, **kw)
            ret += disc * r2.double()                                         # a frozen lane's reward is 0
            disc *= t._discount
        res[name + "_mean_return"] = round(float(ret.mean().item()), 4)
        res[name + "_return_stderr"] = round(float(ret.std().item()) / args.episodes ** .5, 4)
        res[name + "_episodes_ended"] = round(float(t.done.double().mean().item()), 4)
    res.update(tag_episodes=args.episodes, tag_episode_steps=args.episode_steps, tag_ucb_c=10.0, tag_prior_n=args.prior_n)
    if not args.no_resources:
        import kernel_resources as kr
        v = 1 if args.rocks <= 12 else 2
        res["resources"] = [r for r in kr.collect(units=["tree_keep_preferred.hip"]) if r["kernel"] == "tree_resume_preferred_kernel<RockEnv<%d, false> >" % v] + \
                           [r for r in kr.collect(units=["tree_search_preferred.hip"]) if r["kernel"] == "tree_preferred_kernel<RockEnv<%d, false> >" % v] + \
                           [r for r in kr.collect(units=["tree_keep.hip"]) if r["kernel"] == "tree_advance_kernel"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
