"""Stochastic finite-state controllers without a GPU: the C ABI's declaration and every refusal of
pomdp_stoch_controller_episodes (fake device pointers, never dereferenced), the compiled kernels' resources and waits, the host
class gym_pomdp_amd.StochasticController on a stand-in env, and the contract's CPU restatement
(tests/stoch_controller_restatement.py) against the deterministic one and against its own probabilities."""
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
import stoch_controller_restatement as sr  # noqa: E402

BADARG, BADPARAMS = -1, -2
X = 1 << 40                             # a fake, 16-byte aligned "device" address
N = 1000
# the frequency condition's case, shared with test_gpu_stoch_controller.py: Tiger, one node, psi = FREQ_P, FREQ_N lanes, one step
FREQ_SEED, FREQ_N, FREQ_P = 2024, 65536, (.5, .3, .2)


def test_the_entry_point_is_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    assert re.search(r"\bpomdp_stoch_controller_episodes\s*\(", hdr) and "pomdp_stoch_controller_episodes" in _native.SYMBOLS
    assert re.search(r"typedef struct pomdp_stoch_controller\s*\{", hdr)
    assert hdr.index("int pomdp_controller_episodes(") < hdr.index("typedef struct pomdp_stoch_controller") < hdr.index("int pomdp_fuse_max(")
    assert "controller_stoch.hip" in _native.UNITS
    for h in re.findall(r'#include "([^"]+\.hip\.h)"', open(os.path.join(REPO, "gym_pomdp_amd", "csrc", "controller_stoch.hip")).read()):
        assert h in _native.HEADERS, h                                     # a rebuild sees every header the unit reads
    L = _native.lib()
    at = L.pomdp_stoch_controller_episodes.argtypes
    assert len(at) == 5 and at[2] is C.c_uint64 and at[3] is C.c_int64
    assert re.search(r"POMDP_STREAM_CONTROLLER\s*=\s*10\b", hdr) and sr.STREAM_CONTROLLER == 10
    assert re.search(r"POMDP_STREAM_PARTICLE\s*=\s*8\b", hdr) and re.search(r"POMDP_STREAM_TREE\s*=\s*9\b", hdr)
    assert _native.ABI_VERSION == 15 and L.pomdp_abi_version() == 15          # a new entry point only
    assert re.search(r"#define\s+POMDP_ABI_VERSION\s+15\b", hdr)
    assert re.search(r"#define\s+POMDP_STOCH_CONTROLLER_MAX_BYTES\s+36864\b", hdr)


def test_struct_matches_the_header_as_gcc_lays_it_out(tmp_path):
    import subprocess
    from gym_pomdp_amd import _native
    cls = _native.StochController
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pomdp_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(pomdp_stoch_controller));']
    for f in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(pomdp_stoch_controller, %s));' % (f[0], f[0]))
    lines.append('return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    assert [f[0] for f in cls._fields_] == ["action", "action_thr", "next", "next_thr", "n_nodes", "n_obs", "n_act_cand", "n_next_cand", "node"]
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


def _call(env=0, params=None, layout="packed", k=8, n=N, lane0=8, n_nodes=128, n_obs=3, B=3, D=2, null=(), tape=False, pitch=None,
          c_null=False, a_null=False, stats_pitch=None, discount=.95):
    """pomdp_stoch_controller_episodes on valid arguments (RockSample(7, 8), fake device pointers), one thing changed per call"""
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
    c = _native.StochController(action=None if "action" in null else X, action_thr=None if "action_thr" in null else X,
                                next=None if "next" in null else X, next_thr=None if "next_thr" in null else X, n_nodes=n_nodes,
                                n_obs=n_obs, n_act_cand=B, n_next_cand=D, node=None if "node" in null else X)
    return L.pomdp_stoch_controller_episodes(None if a_null else C.byref(a), None if c_null else C.byref(c), (1 << 32) - 3, k, None)


def test_every_refusal_happens_before_anything_is_enqueued():
    from gym_pomdp_amd import _native
    assert _call(k=0) == 0                                                # the call every line below changes one thing of
    # what pomdp_controller_episodes refuses
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
    assert _call(tape=True) == BADARG
    wide = _native.TagParams(num_opponents=1, obs_cells=300, move_thr=1 << 52, move_gt=0, reserved=0)
    assert _call(env=1, params=wide, n_nodes=8, n_obs=301, k=0) == BADPARAMS       # the record keeps the observation in a byte
    assert _call(env=1, params=wide, n_nodes=8, n_obs=301, k=0, layout="returns") == 0
    # the controller's own
    assert _call(c_null=True) == BADARG
    for field in ("action", "next", "node"):
        assert _call(null=(field,)) == BADARG, field
    assert _call(null=("action_thr",)) == _call(null=("next_thr",)) == BADARG      # B = 3, D = 2: both are needed
    assert _call(null=("action_thr",), B=1, k=0) == _call(null=("next_thr",), D=1, k=0) == 0
    assert _call(null=("action_thr", "next_thr"), B=1, D=1, k=0) == 0
    assert _call(null=("action_thr",), B=2) == _call(null=("next_thr",), D=2, B=1) == BADARG
    assert _call(n_nodes=0) == _call(n_nodes=-4) == _call(n_nodes=4097) == BADARG
    assert _call(n_nodes=4096, B=1, D=1, k=0) == 0
    assert _call(B=0) == _call(B=-1) == _call(D=0) == _call(D=-2) == BADARG
    assert _call(B=1 << 30) == _call(D=1 << 30) == _call(B=(1 << 31) - 1, D=(1 << 31) - 1) == BADARG
    assert _call(n_obs=2) == _call(n_obs=4) == _call(n_obs=0) == BADARG   # RockSample observes 3 values
    # the footprint K*B + 4*K*(B-1) + 2*K*O*D + 4*K*O*(D-1): 36864 is the last one taken
    fp = lambda K, O, B, D: K * B + 4 * K * (B - 1) + 2 * K * O * D + 4 * K * O * (D - 1)
    assert fp(512, 3, 14, 1) == 36864 and _call(n_nodes=512, B=14, D=1, k=0) == 0
    assert fp(5, 3, 1467, 3) == 36865 and _call(n_nodes=5, B=1467, D=3, k=0) == BADARG   # one byte past
    assert fp(5, 3, 1466, 3) == 36840 and _call(n_nodes=5, B=1466, D=3, k=0) == 0
    assert fp(1, 3, 7368, 2) == 36860 and _call(n_nodes=1, B=7368, D=2, k=0) == 0        # rounds up to the limit
    assert fp(1, 3, 7369, 2) == 36865 and _call(n_nodes=1, B=7369, D=2, k=0) == BADARG
    assert fp(4096, 3, 1, 1) == 28672 and fp(4096, 3, 2, 1) == 49152 and _call(n_nodes=4096, B=2, D=1, k=0) == BADARG
    tag = _native.TagParams(num_opponents=1, obs_cells=29, move_thr=1 << 52, move_gt=0, reserved=0)
    assert fp(604, 30, 1, 1) == 36844 and _call(env=1, params=tag, n_nodes=604, n_obs=30, B=1, D=1, k=0) == 0
    assert fp(605, 30, 1, 1) == 36905 and _call(env=1, params=tag, n_nodes=605, n_obs=30, B=1, D=1, k=0) == BADARG
    assert _call(env=1, params=tag, n_nodes=604, n_obs=29, B=1, D=1, k=0) == BADARG
    for env, params, n_obs in ((2, _native.BattleShipParams(x_size=5, y_size=5, max_len=3), 2), (3, _native.TigerParams(listen_thr=1 << 52), 3),
                               (4, _native.NetworkParams(n_machines=10), 3)):
        assert _call(env=env, params=params, n_obs=n_obs, k=0) == 0, env
        assert _call(env=env, params=params, n_obs=n_obs + 1, k=0) == BADARG, env


def test_nothing_to_do_returns_zero_without_a_launch():
    for layout in ("packed", "narrow", "returns"):
        assert _call(layout=layout, k=0) == 0
        assert _call(layout=layout, n=0) == 0
        assert _call(layout=layout, k=0, lane0=(1 << 32) - N) == 0       # the last lane is 0xFFFFFFFF


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------
def test_stoch_controller_loops_never_wait_for_their_own_stores(tmp_path):
    """tools/check_loop_waits.py on controller_stoch.hip: no `s_waitcnt vmcnt` in any loop of a kernel — the tables and thresholds
    are staged by straight code before the step loop, the candidate loops read LDS only.  Network's lane step keeps its one
    wait, as in controller_kernel<NetworkEnv, ...>.  Every step loop runs the priority ladder (four s_setprio)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_loop_waits as clw
    res = clw.loop_waits(clw.assembly("controller_stoch.hip", out_dir=str(tmp_path)))
    seen = 0
    for name, (waits, prio) in res.items():
        assert not name.startswith("void pomdp::controller_kernel<"), name
        if not name.startswith("void pomdp::stoch_controller_kernel<"):
            continue
        seen += 1
        assert prio == 4, (name, prio)
        assert len(waits) <= (1 if "NetworkEnv" in name else 0), (name, waits)
    assert seen == 11 * 3, seen                                           # eleven env types x three sinks


def test_stoch_controller_kernels_keep_nothing_in_scratch_and_size_their_tables_per_launch():
    """no scratch (the candidate loops index LDS, not registers); the tables are the launch's dynamic LDS — at most 36 KB, the
    deterministic controller's largest — so what a kernel holds statically is its env's own tables and the reward table, and
    four workgroups still fit a CU"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = [r for r in kr.collect(units=["controller_stoch.hip"]) if r["kernel"].startswith("stoch_controller_kernel<")]
    assert len(rows) == 33
    for r in rows:
        assert r["scratch"] == "0", r
        assert int(r["lds"]) <= 4 * 1024, r
    assert 36864 + 4 * 1024 <= 160 * 1024 // 4


# ---- the host class ------------------------------------------------------------------------------------------------------------
def _stub(n_actions=3, n_obs=3, n=6):
    from gym_pomdp_amd.spaces import Discrete
    return types.SimpleNamespace(action_space=Discrete(n_actions), observation_space=Discrete(n_obs), batch_size=n,
                                 device=torch.device("cpu"), env_name="tiger")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_quantisation_is_the_stated_ceiling():
    from gym_pomdp_amd.stoch_controller import quantise
    q = lambda c0: int(quantise(np.array([c0, 1.0 - c0]))[0])
    assert q(0.0) == 0                                                    # max(0, -1): why a leading zero is refused
    assert q(1.0) == 0xFFFFFFFF                                           # never passed: a probability of 1 is exact
    assert q(2.0 ** -32) == 0                                             # candidate 0 drawn by u = 0 only: 2^-32
    assert q(1.0 - 2.0 ** -33) == 0xFFFFFFFF                              # ceil(2^32 - 1/2) - 1
    assert q(.5) == 0x7FFFFFFF and q(.25) == 0x3FFFFFFF                   # P(u <= thr) = (thr + 1) / 2^32 = c exactly
    assert q(2.0 ** -32 + 2.0 ** -40) == 1                                # the ceiling: just above one step takes two
    t = quantise(np.array([[.5, .3, .2], [.2, 0.0, .8]]))
    assert t.dtype == np.uint32 and t.shape == (2, 2)
    assert t[0].tolist() == [0x7FFFFFFF, int(np.ceil((.5 + .3) * 2.0 ** 32)) - 1]
    assert t[1, 0] == t[1, 1]                                             # a zero in the middle: two equal thresholds, never drawn
    # a cumulative sum that rounding pushed past 1 is clipped
    assert int(quantise(np.array([.7, .3 + 1e-12, 0.0]))[1]) == 0xFFFFFFFF
    # the pick under the thresholds: index 0 for u <= thr[0], the count of thresholds passed after
    u = np.array([0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
    assert sr.pick(u, np.broadcast_to(t[0], (4, 2))).tolist() == [0, 0, 1, 2]


def test_validation_names_the_offending_entry():
    import gym_pomdp_amd as gpa
    e = _stub()
    act, ap = [[0, 1], [2, 0]], [[.5, .5], [1, 0]]
    nxt, nxp = np.zeros((2, 3, 2), int), np.tile([.25, .75], (2, 3, 1))
    c = gpa.StochasticController(e, act, ap, nxt, nxp)
    assert c.action.dtype == c.next.dtype == c.node.dtype == c.action_thr.dtype == torch.int32
    assert c.action.shape == (2, 2) and c.next.shape == (2, 3, 2) and c.action_thr.shape == (2, 1) and c.next_thr.shape == (2, 3, 1)
    assert (c.n_nodes, c.n_obs, c.n_act_cand, c.n_next_cand) == (2, 3, 2, 2) and c.node.tolist() == [0] * 6
    assert _u32(c.action_thr).reshape(-1).tolist() == [0x7FFFFFFF, 0xFFFFFFFF] and (_u32(c.next_thr) == 0x3FFFFFFF).all()
    with pytest.raises(ValueError, match=r"action_p\[1\]\[0\] = 0 stands in front of a positive candidate.*put padding last"):
        gpa.StochasticController(e, act, [[.5, .5], [0, 1]], nxt, nxp)
    with pytest.raises(ValueError, match=r"next_p\[1\]\[2\]\[0\] = 0 .*put padding last"):
        bad = nxp.copy()
        bad[1, 2] = [0, 1]
        gpa.StochasticController(e, act, ap, nxt, bad)
    with pytest.raises(ValueError, match=r"row action_p\[0\] sums to"):
        gpa.StochasticController(e, act, [[.5, .4], [1, 0]], nxt, nxp)
    with pytest.raises(ValueError, match=r"action_p\[0\]\[1\] = -0.5 is negative"):
        gpa.StochasticController(e, act, [[1.5, -.5], [1, 0]], nxt, nxp)
    with pytest.raises(ValueError, match=r"action\[1\]\[0\] = 3 is outside \[0, 3\)"):
        gpa.StochasticController(e, [[0, 1], [3, 0]], ap, nxt, nxp)
    with pytest.raises(ValueError, match=r"next\[0\]\[2\]\[1\] = 2 is outside \[0, 2\)"):
        bad = nxt.copy()
        bad[0, 2, 1] = 2
        gpa.StochasticController(e, act, ap, bad, nxp)
    with pytest.raises(ValueError, match=r"next must have shape \(2, 3, D\)"):
        gpa.StochasticController(e, act, ap, np.zeros((2, 2, 2), int), nxp)
    with pytest.raises(ValueError, match=r"action must have shape \(K, B\)"):
        gpa.StochasticController(e, [0, 1], ap, nxt, nxp)
    with pytest.raises(ValueError, match=r"action_p must hold numbers of shape \(2, 2\)"):
        gpa.StochasticController(e, act, [[1.0], [1.0]], nxt, nxp)
    with pytest.raises(ValueError, match=r"start = 2 is outside \[0, 2\)"):
        gpa.StochasticController(e, act, ap, nxt, nxp, start=2)
    with pytest.raises(ValueError, match=r"past the limits"):
        gpa.StochasticController(e, np.zeros((4097, 1), int), np.ones((4097, 1)), np.zeros((4097, 3, 1), int), np.ones((4097, 3, 1)))
    with pytest.raises(ValueError, match=r"past the limits.*need 36880"):
        gpa.StochasticController(e, np.zeros((5, 1467), int), np.full((5, 1467), 1 / 1467.), np.zeros((5, 3, 3), int), np.full((5, 3, 3), 1 / 3.))
    gpa.StochasticController(e, np.zeros((512, 14), int), np.full((512, 14), 1 / 14.), np.zeros((512, 3, 1), int), np.ones((512, 3, 1)))
    with pytest.raises(ValueError, match=r"validate=False only"):
        gpa.StochasticController(e, act, None, nxt, nxp, action_thr=[[5], [6]])
    # validate=False keeps what the kernel is to refuse and takes the thresholds as they are, monotone or not
    c = gpa.StochasticController(e, [[0, 3, 1 << 32]], None, [[[0, 5], [0, -1], [0, 0]]], None, start=4, validate=False,
                                 action_thr=[[9, 3]], next_thr=[[[0], [0xFFFFFFFF], [7]]])
    assert c.action.tolist() == [[0, 3, -1]] and c.next.tolist() == [[[0, 5], [0, -1], [0, 0]]] and c.node.tolist() == [4] * 6
    assert _u32(c.action_thr).tolist() == [[9, 3]] and _u32(c.next_thr).tolist() == [[[0], [0xFFFFFFFF], [7]]]
    c = gpa.StochasticController(e, [[0, 1]], [[0, 1]], [[[0]] * 3], np.ones((1, 3, 1)), validate=False)   # quantised, unchecked
    assert _u32(c.action_thr).tolist() == [[0]] and c.next_thr.shape == (1, 3, 0)


def test_builders_give_the_stated_shapes_and_padding():
    import gym_pomdp_amd as gpa
    e = _stub()
    det = gpa.Controller(e, [0, 1, 2, 0], [[1, 1, 1], [0, 0, 0], [3, 3, 3], [2, 1, 0]], start=[0, 1, 2, 3, 0, 1])
    c = gpa.StochasticController.from_controller(det)
    assert (c.n_act_cand, c.n_next_cand) == (1, 1) and c.action.tolist() == [[0], [1], [2], [0]] and c.next[:, :, 0].tolist() == det.next.tolist()
    assert c.action_thr.shape == (4, 0) and c.next_thr.shape == (4, 3, 0) and c.node.tolist() == [0, 1, 2, 3, 0, 1]
    name, args = c._native_call()
    assert name == "pomdp_stoch_controller_episodes" and args.action_thr is None and args.next_thr is None and args.n_act_cand == 1
    assert det._native_call()[0] == "pomdp_controller_episodes"
    s = gpa.StochasticController.epsilon_soft(det, .3)
    assert (s.n_act_cand, s.n_next_cand) == (3, 1) and s.next[:, :, 0].tolist() == det.next.tolist() and s.node.tolist() == det.node.tolist()
    assert s.action.tolist() == [[0, 1, 2], [1, 0, 2], [2, 0, 1], [0, 1, 2]]          # the node's own action first
    assert (_u32(s.action_thr) == np.array([int(np.ceil((.7 + .1) * 2.0 ** 32)) - 1, int(np.ceil(((.7 + .1) + .1) * 2.0 ** 32)) - 1])).all()
    z = gpa.StochasticController.epsilon_soft(det, 0.0)                   # the zeros stand last: nothing to refuse
    assert (_u32(z.action_thr) == 0xFFFFFFFF).all()
    with pytest.raises(ValueError, match="eps must lie"):
        gpa.StochasticController.epsilon_soft(det, 1.5)
    psi = np.array([[0.0, .25, .75], [1.0, 0.0, 0.0]])
    eta = np.zeros((2, 3, 2))
    eta[:, :, 1] = 1.0
    eta[1, 2] = [.5, .5]
    d = gpa.StochasticController.from_dense(e, psi, eta, start=1)
    assert (d.n_nodes, d.n_act_cand, d.n_next_cand) == (2, 3, 2) and d.node.tolist() == [1] * 6
    assert d.action.tolist() == [[2, 1, 0], [0, 1, 2]]                    # falling probability, ties by index: zeros last
    assert _u32(d.action_thr).tolist() == [[0xBFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0xFFFFFFFF]]
    assert d.next[0].tolist() == [[1, 0]] * 3 and d.next[1, 2].tolist() == [0, 1] and _u32(d.next_thr)[1, 2].tolist() == [0x7FFFFFFF]
    with pytest.raises(ValueError, match="psi must have shape"):
        gpa.StochasticController.from_dense(e, psi[:, :2], eta)
    parts = [([[0, 1]], [[.5, .5]], [[[0]] * 3], np.ones((1, 3, 1))),
             ([[2], [1]], [[1.0], [1.0]], [[[0, 1]] * 3, [[1, 0]] * 3], np.tile([.25, .75], (2, 3, 1)))]
    u, off = gpa.StochasticController.concat(e, parts)
    assert list(off) == [0, 1] and (u.n_nodes, u.n_act_cand, u.n_next_cand) == (3, 2, 2)
    assert u.action.tolist() == [[0, 1], [2, 2], [1, 1]] and _u32(u.action_thr).reshape(-1).tolist() == [0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    assert u.next.tolist() == [[[0, 0]] * 3, [[1, 2]] * 3, [[2, 1]] * 3]   # shifted with their part; the padding never drawn
    assert _u32(u.next_thr)[0].reshape(-1).tolist() == [0xFFFFFFFF] * 3 and (_u32(u.next_thr)[1:] == 0x3FFFFFFF).all()
    with pytest.raises(ValueError, match=r"next\[0\]\[1\]\[0\] = 1 of part 0 is outside \[0, 1\)"):
        gpa.StochasticController.concat(e, [([[0]], [[1.0]], [[[0], [1], [0]]], np.ones((1, 3, 1)))])


def test_reset_nodes_takes_the_three_forms_of_start():
    import gym_pomdp_amd as gpa
    from gym_pomdp_amd.controller import _LaneNodes
    assert gpa.StochasticController.reset_nodes is _LaneNodes.reset_nodes is gpa.Controller.reset_nodes      # shared, not copied
    assert gpa.StochasticController.start is gpa.Controller.start
    e = _stub()
    mk = lambda start: gpa.StochasticController(e, [[0, 1]] * 4, [[.5, .5]] * 4, np.zeros((4, 3, 1), int), np.ones((4, 3, 1)), start=start)
    where = np.array([1, 0, 0, 1, 0, 1], bool)
    c = mk(2)                                                              # an int
    assert c.node.tolist() == [2] * 6
    c.node.fill_(1)
    assert c.reset_nodes(where=where).tolist() == [2, 1, 1, 2, 1, 2]
    assert c.reset_nodes().tolist() == [2] * 6
    c = mk(torch.tensor([0, 1, 2, 3, 0, 1]))                               # per lane
    assert c.node.tolist() == [0, 1, 2, 3, 0, 1]
    c.node.fill_(3)
    assert c.reset_nodes(where=torch.as_tensor(where)).tolist() == [0, 3, 3, 3, 3, 1]
    c = mk([3, 2, 1])                                                      # a table per reset observation
    assert c.node.tolist() == [0] * 6                                      # nothing observed yet
    with pytest.raises(ValueError, match="StochasticController.reset_nodes: .*pass ob"):
        c.reset_nodes()
    assert c.reset_nodes(ob=np.array([0, 1, 2, 2, 1, 0])).tolist() == [3, 2, 1, 1, 2, 3]
    c.node.fill_(0)
    masked_ob = torch.tensor([2, -1, -1, 0, -1, 1], dtype=torch.int32)    # what reset(where=...) returns: -1 outside the mask
    assert c.reset_nodes(ob=masked_ob, where=where).tolist() == [1, 0, 0, 3, 0, 2]
    with pytest.raises(ValueError, match="start must be"):
        mk([0, 1])


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_restatement_draws_are_the_streams_first_two_words():
    from oracle import philox_ref
    for seed, lane0, t in ((12345, 8, 1), ((1 << 64) - 1, (1 << 32) - 4, (1 << 32) - 1), (7 << 32 | 3, 0, (5 << 32) + 2)):
        u_a, u_n = sr.draws(seed, lane0, 4, t)
        for i in range(4):
            w = philox_ref.stream_words(seed, lane0 + i, t, sr.STREAM_CONTROLLER, 2)
            assert (int(u_a[i]), int(u_n[i])) == (int(w[0]), int(w[1])), (seed, lane0, t, i)
    assert not np.array_equal(sr.draws(1, 0, 4, 1)[0], sr.draws(1, 0, 4, 2)[0])


@pytest.mark.parametrize("env", ["tiger", "rock"])
def test_restatement_with_one_candidate_is_the_deterministic_restatement(oracle_lib, env):
    """B = D = 1: no threshold, every pick is candidate 0 — records, nodes, refused count and statistics are those of
    controller_restatement.run on the same controller, refused entries included (an action out of range, a successor that is
    no node, a lane on no node)"""
    o = oracle_lib.OracleEnv(env)
    n, k, seed, lane0, K = 300, 12, 4242, 8, 9
    rng = np.random.RandomState(5)
    action, nxt = rng.randint(0, o.n_actions, K), rng.randint(0, K, (K, o.n_obs))
    action[7], nxt[8] = o.n_actions, K
    start = rng.randint(0, K, n)
    start[:3] = [7, 8, K]
    res = []
    for stoch in (False, True):
        st = o.new_state(n)
        o.batch_reset(st, seed, lane0, 0)
        done, node = np.zeros(n, np.uint8), start.astype(np.int64)
        acc, cnt = oracle_lib.new_return_stats(n)
        if stoch:
            packed, bad = sr.run(o, st, done, node, action[:, None], np.zeros((K, 0), np.uint32), nxt[:, :, None],
                                 np.zeros((K, o.n_obs, 0), np.uint32), k, seed, lane0, 1, acc, cnt, .95)
        else:
            packed, bad = cr.run(o, st, done, node, action, nxt, k, seed, lane0, 1, acc, cnt, .95)
        res.append((packed, np.array(bad), st, done, node, acc.view(np.uint64), cnt))
    assert res[0][1] >= 3 * 1 and res[0][3].any()
    for x, y in zip(*res):
        assert np.array_equal(x, y)


def frequency_case(ol, seed=FREQ_SEED, n=FREQ_N):
    """the frequency condition's run: Tiger, one node whose three candidates are the three actions with psi = FREQ_P, n lanes,
    one step from a fresh reset -> (how often each action was drawn, the packed row, the state, done)"""
    from gym_pomdp_amd.stoch_controller import quantise
    o = ol.OracleEnv("tiger")
    st = o.new_state(n)
    o.batch_reset(st, seed, 0, 0, nthreads=ol.max_threads())
    done, node = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    packed, bad = sr.run(o, st, done, node, [[0, 1, 2]], quantise(np.array([FREQ_P])), np.zeros((1, 3, 1), int),
                         np.zeros((1, 3, 0), np.uint32), 1, seed, 0, 1, nthreads=ol.max_threads())
    assert bad == 0
    return np.bincount(packed[0] & 0xFF, minlength=3), packed, st, done


def within_five_sigma(counts, n=FREQ_N):
    return all(abs(int(c) - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p)) for c, p in zip(counts, FREQ_P))


def test_restatement_draws_each_action_as_often_as_psi_says(oracle_lib):
    """65 536 lanes, one step: each action's count within 5 sigma (sigma = sqrt(n p (1 - p))) of n p under FREQ_SEED.
    Measured when the test was written: counts (32 901, 19 449, 13 186) against (32 768, 19 660.8, 13 107.2), sigma (128, 117.3,
    102.4): 1.0, 1.8 and 0.8 sigma."""
    counts, _, _, _ = frequency_case(oracle_lib)
    print("counts", counts.tolist())
    assert counts.sum() == FREQ_N and within_five_sigma(counts), counts
