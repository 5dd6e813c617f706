"""Search trees kept between real steps, without a GPU: the C ABI's declarations and argument checks, the workspace size, the
kernels' resources, the pool code under the host sanitizers (tools/tree_keep_hostcheck.cpp, a stand-alone program), and the
contract's CPU restatement (tests/tree_keep_restatement.py) checked on the oracle alone — with the proof that each of the new
rules is pinned by one of its properties."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_keep_restatement as tk  # noqa: E402
import tree_search_restatement as ts  # noqa: E402

NAMES = ("pomdp_tree_keep_workspace", "pomdp_tree_search_resume", "pomdp_tree_advance")


def test_entry_points_are_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    for sym in NAMES:
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in _native.SYMBOLS
        assert hasattr(_native.lib(), sym)
    assert "tree_keep.hip" in _native.UNITS and "tree_keep.hip.h" in _native.HEADERS
    assert _native.ABI_VERSION == 15 and _native.lib().pomdp_abi_version() == 15
    assert re.search(r"#define POMDP_ABI_VERSION 15\b", hdr)
    body = re.search(r"typedef struct pomdp_tree_keep \{(.*?)\} pomdp_tree_keep;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _native.PlanTreeKeep._fields_]
    assert C.sizeof(_native.PlanTreeKeep) == 40 and C.sizeof(_native.PlanTreeArgs) == 200
    import gym_pomdp_amd as gpa
    from gym_pomdp_amd.envs.base import BatchedEnv
    assert callable(BatchedEnv.search_tree) and gpa.SearchTree.__module__ == "gym_pomdp_amd.search_tree"
    for m in ("advance", "clear", "to_host", "n_nodes"):
        assert hasattr(gpa.SearchTree, m)


def _rock_params(num_rocks=8):
    from gym_pomdp_amd import _native
    p = _native.RockParams(size=7, num_rocks=num_rocks, start_x=0, start_y=3)
    for i in range(256):
        p.grid[i] = -1
    for i in range(32):
        p.thr[i] = 1 << 52
    return p


A_, B_, B2_, X, N1, N2 = 1 << 40, 1 << 41, 1 << 43, 1 << 42, 1 << 44, (1 << 44) + (1 << 20)     # fake "device" addresses, aligned
BAD = -1


def test_resume_refuses_bad_arguments_before_any_launch():
    """Every check runs on the host: none of these calls reaches the GPU (fake device pointers are never dereferenced)."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    rock = _rock_params()
    R, W, S, D, Cn = 8, 4, 16, 8, 9                                       # S exceeds C - 1: allowed
    need = L.pomdp_tree_keep_workspace(0, C.byref(rock), R * W, Cn, D)
    assert need > 0

    def call(t0=0, keep=None, no_keep=False, **kw):
        params = kw.pop("params", rock)
        out = dict(q=X, visits=X, best=X, value=None, stride=13, reserved=0)
        out.update(kw.pop("out", {}))
        f = dict(env=0, depth=D, params=None if params is None else C.addressof(params), root_state=A_, particles=None, n_roots=R,
                 n_particles=0, trees_per_root=W, sims_per_tree=S, discount=.95, ucb_c=1.0, logn=X, workspace=None,
                 workspace_bytes=0, tree_visits=X, tree_q=X, n_nodes=X, sim_ret=None, sim_steps=None, sim_tree_steps=None,
                 out=_native.PlanOut(**out), seed=7, lane0=0, reserved=0)
        f.update(kw)
        k = dict(workspace=B_, workspace_bytes=need, n_nodes=N1, node_capacity=Cn, logn_len=S + 1)
        k.update(keep or {})
        return L.pomdp_tree_search_resume(C.byref(_native.PlanTreeArgs(**f)), None if no_keep else C.byref(_native.PlanTreeKeep(**k)),
                                          t0, None)

    assert L.pomdp_tree_search_resume(None, None, 0, None) == BAD
    assert call(no_keep=True) == BAD
    assert call(params=None) == BAD
    for k in ("root_state", "logn", "tree_visits", "tree_q", "n_nodes"):
        assert call(**{k: None}) == BAD, k
    for k in ("q", "visits", "best"):
        assert call(out={k: None}) == BAD, k
    assert call(out=dict(stride=12)) == BAD
    assert call(lane0=2) == BAD and call(n_roots=-1) == call(trees_per_root=0) == call(sims_per_tree=0) == call(depth=-1) == BAD
    for c in (-1.0, float("nan"), float("inf")):
        assert call(ucb_c=c) == BAD, c
    assert call(particles=A_, n_particles=6) == BAD and call(n_particles=8) == BAD
    assert call(env=9) == BAD
    bad_rock = _rock_params()
    bad_rock.size = 99
    assert call(params=bad_rock) == -2
    # the kept trees
    assert call(keep=dict(workspace=None)) == BAD
    assert call(keep=dict(n_nodes=None)) == BAD
    assert call(keep=dict(workspace=B_ + 8)) == BAD                       # misaligned
    assert call(keep=dict(workspace_bytes=need - 1)) == BAD               # short
    assert call(keep=dict(node_capacity=0)) == call(keep=dict(node_capacity=-3)) == BAD
    assert call(keep=dict(node_capacity=(1 << 31) // 13 + 1, workspace_bytes=1 << 60)) == BAD     # C * A >= 2^31
    assert call(keep=dict(logn_len=1)) == call(keep=dict(logn_len=0)) == call(keep=dict(logn_len=-5)) == BAD
    assert call(keep=dict(logn_len=(1 << 31) // W + 1)) == BAD            # W * (logn_len - 1) > 2^31 - 1
    # what pomdp_tree_search's own rules no longer cover: a->workspace is ignored
    assert call(n_roots=0) == 0 and call(n_roots=0, keep=dict(workspace=None, workspace_bytes=0)) == 0


def test_advance_refuses_bad_arguments_before_any_launch():
    from gym_pomdp_amd import _native
    L = _native.lib()
    rock = _rock_params()
    R, W, D, Cn = 8, 4, 8, 9
    need = L.pomdp_tree_keep_workspace(0, C.byref(rock), R * W, Cn, D)

    def keep(**kw):
        k = dict(workspace=B_, workspace_bytes=need, n_nodes=N1, node_capacity=Cn, logn_len=2)
        k.update(kw)
        return _native.PlanTreeKeep(**k)

    def call(src=None, dst=None, env=0, params=rock, n_roots=R, W=W, D=D, action=X, ob=X, drop=None):
        src = keep() if src is None else src
        dst = keep(workspace=B2_, n_nodes=N2) if dst is None else dst
        return L.pomdp_tree_advance(env, None if params is None else C.byref(params), n_roots, W, D,
                                    None if src == "null" else C.byref(src), None if dst == "null" else C.byref(dst), action, ob, drop, None)

    assert call(params=None) == BAD and call(src="null") == BAD and call(dst="null") == BAD
    assert call(action=None) == BAD and call(ob=None) == BAD
    assert call(env=9) == BAD and call(n_roots=-1) == BAD and call(W=0) == BAD and call(D=-1) == BAD
    for side in ("src", "dst"):
        base = dict(workspace=B2_, n_nodes=N2) if side == "dst" else {}
        for kw in (dict(workspace=None), dict(n_nodes=None), dict(workspace=base.get("workspace", B_) + 8), dict(workspace_bytes=need - 1),
                   dict(node_capacity=0), dict(node_capacity=(1 << 31) // 13 + 1, workspace_bytes=1 << 60)):
            d = dict(base)
            d.update(kw)
            assert call(**{side: keep(**d)}) == BAD, (side, kw)
    same = keep()
    assert call(src=same, dst=same) == BAD                                # src == dst
    assert call(dst=keep(n_nodes=N2)) == BAD                              # the same workspace
    assert call(dst=keep(workspace=B_ + need - 16, n_nodes=N2)) == BAD    # overlapping workspaces
    assert call(dst=keep(workspace=B2_, n_nodes=N1 + 4 * (R * W - 1))) == BAD      # overlapping counts
    assert call(dst=keep(workspace=B2_, n_nodes=N2, node_capacity=Cn + 1, workspace_bytes=1 << 40)) == BAD     # a mismatched C
    bad_rock = _rock_params()
    bad_rock.size = 99
    assert call(params=bad_rock) == -2
    assert call(n_roots=0) == 0
    assert call(n_roots=0, src=keep(workspace=None, workspace_bytes=0), dst=keep(workspace=None, workspace_bytes=0, n_nodes=N2)) == 0


def test_workspace_size_is_monotone_and_zero_for_refused_shapes():
    from gym_pomdp_amd import _native
    L = _native.lib()
    ws = lambda K=8, n=32, Cn=17, D=8: L.pomdp_tree_keep_workspace(0, C.byref(_rock_params(K)), n, Cn, D)
    base = ws()
    assert base > 0 and base % 16 == 0
    assert base == 32 * 16 * (17 * 13 + 17 + 8)                           # edge [C][A], node [C], path [min(D, C)]
    assert ws(K=9) > base and ws(n=33) > base and ws(Cn=18) > base
    assert ws(D=9) > base and ws(D=17) > ws(D=16) and ws(D=18) == ws(D=17)      # the path never outgrows min(D, C) entries
    for n in range(0, 5):
        assert ws(n=n) == n * ws(n=1)
    assert [ws(Cn=c) for c in range(1, 40)] == sorted(ws(Cn=c) for c in range(1, 40))
    assert [ws(D=d) for d in range(0, 40)] == sorted(ws(D=d) for d in range(0, 40))
    assert all(ws(Cn=c, D=d) % 16 == 0 for c in (1, 2, 33) for d in (0, 1, 40))
    assert ws(Cn=1, D=0, n=1) == 16 * (13 + 1)
    assert ws(n=-1) == ws(Cn=0) == ws(Cn=-1) == ws(D=-1) == ws(n=(1 << 32) + 1) == 0
    assert ws(Cn=(1 << 31) // 13 + 1, n=1) == 0 and ws(Cn=(1 << 31) // 13, n=1) > 0      # C * A >= 2^31 / just below
    assert L.pomdp_tree_keep_workspace(0, None, 32, 17, 8) == L.pomdp_tree_keep_workspace(9, C.byref(_rock_params()), 32, 17, 8) == 0
    assert ws(n=1 << 32, Cn=1 << 20, D=64) == 0                           # more than any device holds: refused, not wrapped


def test_tree_keep_kernels_keep_nothing_in_scratch_memory():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = kr.collect(units=["tree_keep.hip"])
    names = [r["kernel"] for r in rows]
    assert sum(1 for k in names if k.startswith("tree_resume_kernel<")) == 11          # per env type
    assert names.count("tree_advance_kernel") == 1
    assert not [k for k in names if k.startswith("tree_search_kernel")]                # new kernel names only
    bad = [(r["kernel"], r["scratch"]) for r in rows if r["scratch"] != "0"]
    assert not bad, bad


def test_pool_code_under_the_host_sanitizers(tmp_path):
    """tools/tree_keep_hostcheck.cpp: its own main, tree_keep.hip.h included as it is, pools of exactly the advertised bytes;
    built with g++ -fsanitize=address,undefined and run as a child process."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "tree_keep_hostcheck")
    cc = subprocess.run([gxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-o", exe,
                         os.path.join(REPO, "tools", "tree_keep_hostcheck.cpp")], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", cc.stderr):
        pytest.skip("g++ has no sanitizer runtime")
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "tree_keep_hostcheck: ok" in run.stdout


# ---- the restatement on the oracle alone ------------------------------------------------------------------------------------
SEED = 77
KEYS = ("tree_visits", "tree_q", "n_nodes", "sim_ret", "sim_steps", "sim_tree_steps", "q", "visits", "best", "value")


def _reset(o, n, seed=5):
    st = o.new_state(n)
    o.batch_reset(st, seed, 0, 0)
    return st


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("env,kw", [("tiger", {}), ("rock", {}), ("tag", {})])
def test_resume_from_empty_equals_the_search(env, kw):
    """the anchor: empty trees, C = S + 1, logn_len = S + 1 — every output of ts.search, bit for bit"""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv(env, **kw)
    R, W, S, D = 5, 2, 20, 8
    roots = _reset(o, R)
    want = ts.search(o, roots, R, W, S, D, .95, 3.0, SEED, 4, 9)
    got = tk.search(o, roots, R, W, S, D, .95, 3.0, SEED, 4, 9)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert not got["full"].any()
    for t in got["trees"]:
        assert all(int(t.N[h].sum()) == t.Nh[h] for h in range(len(t.N)))


def _tiger_steps(mutate=None, C=67, steps=3, drop_at=None):
    """Tiger (LISTEN is the best action for a while, two observations): searches of 4 x 3 trees with the real step between
    them -> per step the search result, the trees' sizes and canonical forms before the advance, the trees after it (a later
    search grows them in place: after_sizes and after_ok were taken at once), action, ob, drop"""
    from oracle import oracle_lib as ol
    o = ol.OracleEnv("tiger")
    R, W, S, D = 4, 3, 33, 10
    st = _reset(o, R)
    trees, t, rec = None, 100, []
    logn = ts.log_table(steps * S)
    for step in range(steps):
        res = tk.search(o, st, R, W, S, D, .95, 10.0, SEED, 0, t, trees=trees, C=C, logn=logn, mutate=mutate)
        t += S * D
        a = res["best"].copy()
        ob, rew, done, _ = o.batch_step(st, a, SEED, 0, t, auto_reset=False)
        t += 1
        drop = np.zeros(R, np.uint8)
        if drop_at == step:
            drop[1] = 1
        before = res["trees"]
        sizes = tk.n_nodes_of(before)
        canon_before = [tk.canon(x) for x in before]
        trees = tk.advance(before, W, a, ob, drop, mutate=mutate)
        rec.append(dict(res=res, sizes=sizes, canon_before=canon_before, after=trees, after_sizes=tk.n_nodes_of(trees),
                        after_ok=[t is None or all(int(t.N[h].sum()) == t.Nh[h] for h in range(len(t.N))) for t in trees],
                        a=a, ob=ob, drop=drop))
    return R, W, S, rec


def prop_no_match_empties_the_tree(mutate=None):
    """An observation the root's action never produced in a tree's simulations leaves that tree nothing to keep: advancing under
    (a, an observation no tree has seen) gives empty trees everywhere, and a kept tree is exactly the child's subtree.
    Mutation that fails it: the no-match branch hands the old tree back (no_match_keeps_root)."""
    R, W, S, rec = _tiger_steps(steps=1)
    before = rec[0]["res"]["trees"]
    none = tk.advance(before, W, rec[0]["a"], np.full(R, 99, np.int32), mutate=mutate)
    assert all(t is None for t in none) and (tk.n_nodes_of(none) == 0).all()
    kept = tk.advance(before, W, rec[0]["a"], rec[0]["ob"], mutate=mutate)
    assert any(t is not None for t in kept)
    for i, t in enumerate(kept):
        a, ob = int(rec[0]["a"][i // W]), int(rec[0]["ob"][i // W])
        want = {p[1:]: v for p, v in rec[0]["canon_before"][i].items() if p[:1] == ((a, ob),)}
        assert tk.same_canon(tk.canon(t), want)
        assert (0 if t is None else len(t.N)) == len(want)


def prop_drop_empties_the_tree(mutate=None):
    """drop[r] != 0 empties every tree of root r whatever it holds, and only those.
    Mutation that fails it: drop is not looked at (drop_ignored)."""
    R, W, S, rec = _tiger_steps(steps=1)
    before = rec[0]["res"]["trees"]
    plain = tk.advance(before, W, rec[0]["a"], rec[0]["ob"])
    assert any(plain[i] is not None for i in range(W, 2 * W))             # root 1 had something to keep
    drop = np.array([0, 1, 0, 0], np.uint8)
    got = tk.advance(before, W, rec[0]["a"], rec[0]["ob"], drop, mutate=mutate)
    for i in range(R * W):
        if i // W == 1:
            assert got[i] is None
        else:
            assert tk.same_canon(tk.canon(got[i]), tk.canon(plain[i]))


def prop_a_full_pool_rolls_out_without_a_node(mutate=None):
    """C = 20 over three searches of S = 33: the pools fill up within the first search; a tree never holds more than C nodes,
    and the simulations that met the full pool still ran (every simulation took a step and was backed up).
    Mutation that fails it: the node is created all the same (full_pool_creates)."""
    R, W, S, rec = _tiger_steps(mutate=mutate, C=20, steps=3)
    assert sum(int(r["res"]["full"].sum()) for r in rec) > 0
    for r in rec:
        assert (r["sizes"] <= 20).all()
        assert (r["res"]["sim_steps"] > 0).all()
        for i, c in enumerate(r["canon_before"]):
            assert len(c) == r["sizes"][i]


def prop_nh_is_carried_into_the_new_root(mutate=None):
    """Every node's Nh is sum_a N(h,a) — before and after an advance, the new root included — and after the second search the
    root's Nh exceeds S: the log table is read past entry S.
    Mutation that fails it: the new root's Nh restarts at 0 (nh_not_carried)."""
    R, W, S, rec = _tiger_steps(mutate=mutate, steps=3)
    seen_big = False
    for r in rec:
        assert all(r["after_ok"])
        for c in r["canon_before"]:
            seen_big |= c[()][2] > S
            assert c[()][2] == int(c[()][0].sum())
    assert seen_big


PROPS = {"no_match_keeps_root": prop_no_match_empties_the_tree,
         "drop_ignored": prop_drop_empties_the_tree,
         "full_pool_creates": prop_a_full_pool_rolls_out_without_a_node,
         "nh_not_carried": prop_nh_is_carried_into_the_new_root}


@pytest.mark.parametrize("rule", list(PROPS))
def test_restatement_property(rule):
    PROPS[rule]()


@pytest.mark.parametrize("rule", list(PROPS))
def test_every_new_rule_is_pinned_by_a_property(rule):
    """One one-token mutation per new rule (tree_keep_restatement.MUTATIONS; each property's docstring names its own): the
    property that holds for the restatement as written fails for the mutant."""
    assert set(PROPS) == set(tk.MUTATIONS)
    with pytest.raises(AssertionError):
        PROPS[rule](mutate=rule)


def test_kept_trees_keep_their_statistics_across_the_real_step():
    """Tiger, three real steps at C = 67: some tree keeps at least 8 nodes, no pool fills, and the visits of the root after the
    second search are the kept child's plus S."""
    R, W, S, rec = _tiger_steps(steps=3)
    assert max(int(r["after_sizes"].max()) for r in rec) >= 8
    assert not any(r["res"]["full"].any() for r in rec)
    for prev, cur in zip(rec, rec[1:]):
        for i in range(R * W):
            kept = 0 if prev["after_sizes"][i] == 0 else int(prev["canon_before"][i][((int(prev["a"][i // W]), int(prev["ob"][i // W])),)][2])
            assert cur["canon_before"][i][()][2] == kept + S
