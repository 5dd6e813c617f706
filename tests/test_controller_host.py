"""Finite-state controllers without a GPU: the C ABI's declaration and every refusal of pomdp_controller_episodes (fake device
pointers, never dereferenced), the compiled kernels' resources and waits, the host class gym_pomdp_amd.Controller on a stand-in
env, and the contract's CPU restatement (tests/controller_restatement.py) against a plain loop over the oracle."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import controller_restatement as cr  # noqa: E402

BADARG, BADPARAMS = -1, -2
X = 1 << 40                             # a fake, 16-byte aligned "device" address
N = 1000


def test_the_entry_point_is_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    assert re.search(r"\bpomdp_controller_episodes\s*\(", hdr) and "pomdp_controller_episodes" in _native.SYMBOLS
    assert re.search(r"typedef struct pomdp_controller\s*\{", hdr)
    assert hdr.index("int pomdp_finish_episodes(") < hdr.index("typedef struct pomdp_controller") < hdr.index("int pomdp_fuse_max(")
    assert "controller.hip" in _native.UNITS
    L = _native.lib()
    at = L.pomdp_controller_episodes.argtypes
    assert len(at) == 5 and at[2] is C.c_uint64 and at[3] is C.c_int64
    assert _native.ABI_VERSION == 15 and L.pomdp_abi_version() == 15          # a new entry point only
    assert re.search(r"#define\s+POMDP_ABI_VERSION\s+15\b", hdr)


def test_controller_struct_matches_the_header_as_gcc_lays_it_out(tmp_path):
    import subprocess
    from gym_pomdp_amd import _native
    cls = _native.Controller
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pomdp_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(pomdp_controller));']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(pomdp_controller, %s));' % (f[0], f[0]))
    lines.append('return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _rock_params():
    from gym_pomdp_amd import _native
    p = _native.RockParams(size=7, num_rocks=8, start_x=0, start_y=3)
    for i in range(256):
        p.grid[i] = -1
    for i in range(32):
        p.thr[i] = 1 << 52
    return p


def _call(env=0, params=None, layout="packed", k=8, n=N, lane0=8, n_nodes=128, n_obs=3, null=(), tape=False, pitch=None, c_null=False,
          a_null=False, stats_pitch=None, discount=.95):
    """pomdp_controller_episodes on valid arguments (RockSample(7, 8), fake device pointers), one thing changed per call"""
    from gym_pomdp_amd import _native
    L = _native.lib()
    params = _rock_params() if params is None else params
    rets = layout == "returns"
    tp = _native.Tape(actions=X, stride=n)
    st = _native.ReturnStats(discount, None if "acc" in null else X, None if "cnt" in null else X, n if stats_pitch is None else stats_pitch)
    a = _native.EpisodeArgs(env=env, layout=_native.POMDP_LAYOUT_RETURNS if rets else _native.LAYOUTS.get(layout, 7),
                            params=None if "params" in null else C.addressof(params), state=None if "state" in null else X,
                            done=None if "done" in null else X, tape=C.addressof(tp) if tape else None,
                            traj=None if rets or "traj" in null else X, pitch=n if pitch is None else pitch,
                            stats=C.addressof(st) if rets and "stats" not in null else None, err=None, n=n, seed=7, lane0=lane0, reserved=0)
    c = _native.Controller(action=None if "action" in null else X, next=None if "next" in null else X, n_nodes=n_nodes, n_obs=n_obs,
                           node=None if "node" in null else X)
    return L.pomdp_controller_episodes(None if a_null else C.byref(a), None if c_null else C.byref(c), (1 << 32) - 3, k, None)


def test_every_refusal_happens_before_anything_is_enqueued():
    from gym_pomdp_amd import _native
    # what pomdp_finish_episodes refuses
    assert _call(a_null=True) == BADARG
    for field in ("params", "state", "done"):
        assert _call(null=(field,)) == BADARG, field
    assert _call(k=-1) == BADARG
    assert _call(lane0=6) == BADARG                                       # lane0 % 4
    assert _call(lane0=(1 << 32) - N + 4) == BADARG                      # lane0 + n > 2^32
    assert _call(n=-1) == BADARG
    assert _call(layout="returns", null=("stats",)) == _call(layout="returns", null=("acc",)) == _call(layout="returns", null=("cnt",)) == BADARG
    assert _call(layout="returns", stats_pitch=N - 1) == _call(layout="returns", discount=float("nan")) == BADARG
    assert _call(null=("traj",)) == _call(pitch=N - 1) == BADARG
    assert _call(layout="narrow", pitch=N + 2) == BADARG                  # Narrow planes on 4-byte boundaries
    assert _call(layout="columns") == _call(layout="blocked") == _call(layout="none") == BADARG
    assert _call(env=9) == BADARG                                         # unknown env
    bad_rock = _rock_params()
    bad_rock.size = 16
    assert _call(params=bad_rock) == BADPARAMS
    # the controller's own
    assert _call(c_null=True) == BADARG
    for field in ("action", "next", "node"):
        assert _call(null=(field,)) == BADARG, field
    assert _call(n_nodes=0) == _call(n_nodes=-4) == _call(n_nodes=4097) == BADARG
    assert _call(n_obs=2) == _call(n_obs=4) == _call(n_obs=0) == BADARG   # RockSample observes 3 values
    assert _call(tape=True) == BADARG
    tag = _native.TagParams(num_opponents=1, obs_cells=29, move_thr=1 << 52, move_gt=0, reserved=0)
    assert _call(env=1, params=tag, n_nodes=547, n_obs=30, k=0) == BADARG          # 16 410 successors
    assert _call(env=1, params=tag, n_nodes=546, n_obs=30, k=0) == 0               # 16 380
    assert _call(env=1, params=tag, n_nodes=546, n_obs=29, k=0) == BADARG
    wide = _native.TagParams(num_opponents=1, obs_cells=300, move_thr=1 << 52, move_gt=0, reserved=0)
    assert _call(env=1, params=wide, n_nodes=8, n_obs=301, k=0) == BADPARAMS       # the record keeps the observation in a byte
    assert _call(env=1, params=wide, n_nodes=8, n_obs=301, k=0, layout="returns") == 0
    for env, params, n_obs in ((2, _native.BattleShipParams(x_size=5, y_size=5, max_len=3), 2), (3, _native.TigerParams(listen_thr=1 << 52), 3),
                               (4, _native.NetworkParams(n_machines=10), 3)):
        assert _call(env=env, params=params, n_obs=n_obs, k=0) == 0, env
        assert _call(env=env, params=params, n_obs=n_obs + 1, k=0) == BADARG, env


def test_nothing_to_do_returns_zero_without_a_launch():
    for layout in ("packed", "narrow", "returns"):
        assert _call(layout=layout, k=0) == 0
        assert _call(layout=layout, n=0) == 0
        assert _call(layout=layout, k=0, n_nodes=4096) == 0              # the largest RockSample controller: 12 288 successors
        assert _call(layout=layout, k=0, lane0=(1 << 32) - N) == 0       # the last lane is 0xFFFFFFFF


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------
def test_controller_loops_never_wait_for_their_own_stores(tmp_path):
    """tools/check_loop_waits.py on controller.hip: no `s_waitcnt vmcnt` in any loop of a controller kernel — the tables are
    staged by straight code before the step loop, which itself holds no load (a wait there would stall every step on the
    previous step's stores).  Network's lane step reads its thresholds from the kernel arguments inside its per-lane draw loop,
    one wait there, as in episodes_kernel<NetworkEnv, ...>.  Every step loop runs the priority ladder (four s_setprio)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_loop_waits as clw
    res = clw.loop_waits(clw.assembly("controller.hip", out_dir=str(tmp_path)))
    seen = 0
    for name, (waits, prio) in res.items():
        if not name.startswith("void pomdp::controller_kernel<"):
            continue
        seen += 1
        assert prio == 4, (name, prio)
        assert len(waits) <= (1 if "NetworkEnv" in name else 0), (name, waits)
    assert seen == 11 * 3, seen                                           # eleven env types x three sinks


def test_controller_kernels_keep_nothing_in_scratch_and_size_their_tables_per_launch():
    """no scratch; the tables are the launch's dynamic LDS (a halfword per successor, a byte per node: 36 KB for the largest
    controller, four workgroups per CU), so what a kernel holds statically is its env's own tables and the reward table"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = [r for r in kr.collect(units=["controller.hip"]) if r["kernel"].startswith("controller_kernel<")]
    assert len(rows) == 33
    for r in rows:
        assert r["scratch"] == "0", r
        assert int(r["lds"]) <= 4 * 1024, r
    assert 2 * 16384 + 4096 + 4 * 1024 <= 160 * 1024 // 4


# ---- the host class ------------------------------------------------------------------------------------------------------------
def _stub(n_actions=3, n_obs=3, n=6):
    from gym_pomdp_amd.spaces import Discrete
    return types.SimpleNamespace(action_space=Discrete(n_actions), observation_space=Discrete(n_obs), batch_size=n,
                                 device=torch.device("cpu"), env_name="tiger")


def test_controller_validation_names_the_offending_entry():
    import gym_pomdp_amd as gpa
    e = _stub()
    ok_next = [[1, 1, 1], [0, 0, 0]]
    c = gpa.Controller(e, [0, 1], ok_next)
    assert c.action.dtype == c.next.dtype == c.node.dtype == torch.int32 and c.next.shape == (2, 3) and c.node.shape == (6,)
    with pytest.raises(ValueError, match=r"action\[1\] = 3 is outside \[0, 3\)"):
        gpa.Controller(e, [0, 3], ok_next)
    with pytest.raises(ValueError, match=r"action\[0\] = -1 "):
        gpa.Controller(e, [-1, 3], ok_next)
    with pytest.raises(ValueError, match=r"next\[1\]\[2\] = 2 is outside \[0, 2\)"):
        gpa.Controller(e, [0, 1], [[1, 1, 1], [0, 0, 2]])
    with pytest.raises(ValueError, match=r"next must have shape \(2, 3\)"):
        gpa.Controller(e, [0, 1], [[1, 1], [0, 0]])
    with pytest.raises(ValueError, match=r"action must have shape"):
        gpa.Controller(e, [[0, 1]], ok_next)
    with pytest.raises(ValueError, match=r"integers"):
        gpa.Controller(e, [0., 1.], ok_next)
    with pytest.raises(ValueError, match=r"start = 2 is outside \[0, 2\)"):
        gpa.Controller(e, [0, 1], ok_next, start=2)
    with pytest.raises(ValueError, match=r"start\[4\] = 7 is outside"):
        gpa.Controller(e, [0, 1], ok_next, start=[0, 1, 0, 1, 7, 0])
    with pytest.raises(ValueError, match=r"past the limits"):
        gpa.Controller(e, np.zeros(4097, int), np.zeros((4097, 3), int))
    with pytest.raises(ValueError, match=r"past the limits"):
        gpa.Controller(_stub(n_obs=30), np.zeros(547, int), np.zeros((547, 30), int))
    gpa.Controller(_stub(n_obs=30), np.zeros(546, int), np.zeros((546, 30), int))
    gpa.Controller(e, np.zeros(4096, int), np.zeros((4096, 3), int))
    # validate=False keeps what the kernel is to refuse; a value outside int32 becomes -1 instead of wrapping into range
    c = gpa.Controller(e, [0, 3, 1 << 32], [[1, 1, 1], [0, 0, 2], [0, 0, -5]], start=3, validate=False)
    assert c.action.tolist() == [0, 3, -1] and c.next.tolist() == [[1, 1, 1], [0, 0, 2], [0, 0, -5]] and c.node.tolist() == [3] * 6


def test_concat_is_the_disjoint_union_with_shifted_successors():
    import gym_pomdp_amd as gpa
    e = _stub()
    parts = [([0, 1], [[1, 1, 1], [0, 0, 0]]), ([2], [[0, 0, 0]]), ([1, 1, 0], [[2, 1, 0], [0, 0, 0], [1, 2, 2]])]
    c, off = gpa.Controller.concat(e, parts)
    assert list(off) == [0, 2, 3] and c.n_nodes == 6
    assert c.action.tolist() == [0, 1, 2, 1, 1, 0]
    assert c.next.tolist() == [[1, 1, 1], [0, 0, 0], [2, 2, 2], [5, 4, 3], [3, 3, 3], [4, 5, 5]]
    with pytest.raises(ValueError, match=r"next\[0\]\[1\] = 1 of part 1 is outside \[0, 1\)"):
        gpa.Controller.concat(e, [parts[0], ([2], [[0, 1, 0]])])
    m = gpa.Controller.memoryless(e, [2, 0, 1], first_action=0)
    assert m.action.tolist() == [2, 0, 1, 0] and m.next.tolist() == [[0, 1, 2]] * 4 and m.node.tolist() == [3] * 6
    o = gpa.Controller.open_loop(e, [0, 0, 2])
    assert o.action.tolist() == [0, 0, 2] and o.next.tolist() == [[1] * 3, [2] * 3, [2] * 3] and o.node.tolist() == [0] * 6
    assert gpa.Controller.open_loop(e, [0, 0, 2], loop=True).next.tolist() == [[1] * 3, [2] * 3, [0] * 3]


def test_reset_nodes_takes_the_three_forms_of_start():
    import gym_pomdp_amd as gpa
    e = _stub()
    action, nxt = [0, 1, 2, 0], np.zeros((4, 3), int)
    where = np.array([1, 0, 0, 1, 0, 1], bool)
    c = gpa.Controller(e, action, nxt, start=2)                           # an int
    assert c.node.tolist() == [2] * 6
    c.node.fill_(1)
    assert c.reset_nodes(where=where).tolist() == [2, 1, 1, 2, 1, 2]
    assert c.reset_nodes().tolist() == [2] * 6
    c = gpa.Controller(e, action, nxt, start=torch.tensor([0, 1, 2, 3, 0, 1]))      # per lane
    assert c.node.tolist() == [0, 1, 2, 3, 0, 1]
    c.node.fill_(3)
    assert c.reset_nodes(where=torch.as_tensor(where)).tolist() == [0, 3, 3, 3, 3, 1]
    c = gpa.Controller(e, action, nxt, start=[3, 2, 1])                   # a table per reset observation
    assert c.node.tolist() == [0] * 6                                     # nothing observed yet
    with pytest.raises(ValueError, match="pass ob"):
        c.reset_nodes()
    assert c.reset_nodes(ob=np.array([0, 1, 2, 2, 1, 0])).tolist() == [3, 2, 1, 1, 2, 3]
    c.node.fill_(0)
    masked_ob = torch.tensor([2, -1, -1, 0, -1, 1], dtype=torch.int32)   # what reset(where=...) returns: -1 outside the mask
    assert c.reset_nodes(ob=masked_ob, where=where).tolist() == [1, 0, 0, 3, 0, 2]
    with pytest.raises(ValueError, match="start must be"):
        gpa.Controller(e, action, nxt, start=[0, 1])
    c.start = 1
    assert c.reset_nodes().tolist() == [1] * 6


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", ["rock", "tiger", "tag"])
def test_restatement_under_an_open_loop_controller_is_a_plain_step_loop(oracle_lib, env):
    """a chain of K nodes whose successors ignore the observation takes actions[s] at step s: the rows, the final state and the
    done flags are those of batch_step over the same actions; the node ends on min(steps taken, K - 1)"""
    o = oracle_lib.OracleEnv(env)
    n, k, seed, lane0 = 300, 12, 4242, 8
    rng = np.random.RandomState(3)
    actions = rng.randint(0, o.n_actions, k)
    nxt = np.repeat(np.minimum(np.arange(1, k + 1), k - 1)[:, None], o.n_obs, axis=1)
    st = o.new_state(n)
    o.batch_reset(st, seed, lane0, 0)
    ref, ref_done = st.copy(), np.zeros(n, np.uint8)
    done, node = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    packed, bad = cr.run(o, st, done, node, actions, nxt, k, seed, lane0, 1)
    assert bad == 0
    taken = np.zeros(n, np.int64)
    for s in range(k):
        live = ref_done == 0
        ob, rw, d, b = o.batch_step(ref, np.full(n, actions[s], np.int32), seed, lane0, 1 + s, auto_reset=False, done=ref_done)
        taken += live
        assert b == 0
        assert ((packed[s] & 0xFF)[live] == actions[s]).all()
        assert np.array_equal((packed[s] >> 8 & 0xFF)[live], ob[live]) and np.array_equal(packed[s] >> 24, d)
        assert np.array_equal(cr.code_reward(env, packed[s] >> 16)[live], rw[live].astype(np.float64))
        assert (packed[s][~live] >> 8 == 1 << 16).all()                   # frozen rows: (ob, reward, done) = (0, 0, 1)
    assert np.array_equal(st, ref) and np.array_equal(done, ref_done)
    assert np.array_equal(node, np.minimum(taken, k - 1))
    # a frozen lane's action byte is its node's action: the node it stopped on
    s_last = k - 1
    frozen = taken < k
    assert np.array_equal((packed[s_last] & 0xFF)[frozen], actions[np.minimum(taken, k - 1)][frozen])


def test_restatement_rules_for_refused_entries(oracle_lib):
    """Tiger, three lanes on a two-node controller that holds an action out of range, a successor that is no node, and a lane
    that stands on no node: untouched or stays, counted, as the header says"""
    o = oracle_lib.OracleEnv("tiger")
    n, seed = 4, 9
    st = o.new_state(n)
    o.batch_reset(st, seed, 0, 0)
    st0 = st.copy()
    action = np.array([0, 3, 300])                                        # open door 0; out of range; does not fit a byte
    nxt = np.array([[0, 0, 7], [1, 1, 1], [2, 2, 2]])                     # node 0 on observation 2: no node 7
    node = np.array([0, 1, 2, 5], np.int64)                               # lane 3 stands on no node
    done = np.zeros(n, np.uint8)
    acc, cnt = np.zeros((4, n)), np.zeros((2, n), np.int64)
    acc[1] = 1.0
    packed, bad = cr.run(o, st, done, node, action, nxt, 3, seed, 0, 1, acc, cnt, .5)
    assert np.array_equal(packed[:, 1], [3, 3, 3]) and np.array_equal(packed[:, 2], [255, 255, 255]) and np.array_equal(packed[:, 3], [255] * 3)
    assert np.array_equal(st[:, 1:], st0[:, 1:]) and not done[1:].any() and node.tolist()[1:] == [1, 2, 5]
    assert node[0] == 0 and bad == 9 + int((packed[:, 0] >> 8 & 0xFF == 2).sum())
    assert np.array_equal(cnt[1][1:], [3, 3, 3]) and np.array_equal(acc[0][1:], [0, 0, 0]) and np.array_equal(acc[1][1:], [.125] * 3)
