"""pomdp_heuristic_collect / env.collect_heuristic without a GPU: the symbol, the arguments the entry point refuses before any
launch, and the Python-side checks that fire before the device is touched."""
import ctypes as C
import os
import re
import types

import pytest

from conftest import REPO


def test_the_symbol_is_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    header = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    assert re.search(r"^int pomdp_heuristic_collect\(", header, re.M)
    assert "#define POMDP_ABI_VERSION 15" in header and _native.ABI_VERSION == 15         # a new entry point only
    assert "pomdp_heuristic_collect" in _native.SYMBOLS
    assert "heuristic_collect.hip" in _native.UNITS and "heuristic_impl.hip.h" in _native.HEADERS
    L = _native.lib()
    assert hasattr(L, "pomdp_heuristic_collect") and len(L.pomdp_heuristic_collect.argtypes) == 21


def _args(**over):
    """A call nothing is wrong with for Tag — host memory stands in for the device arrays: no launch ever reads it here."""
    from gym_pomdp_amd import _native
    keep = [(C.c_uint64 * 64)() for _ in range(10)]
    ptr = [C.cast(k, C.c_void_p) for k in keep]
    params = _native.TagParams(num_opponents=1, obs_cells=29)
    hist = _native.HistoryPtrs(size=ptr[0].value, last_action=ptr[1].value, last_ob=ptr[2].value, max_size=-1)
    a = dict(env=_native.ENV_KIND["tag"], params=C.byref(params), state=ptr[3], b=None, h=C.byref(hist), prev_ob=ptr[4], action=ptr[5],
             ob=ptr[6], reward=ptr[7], done=ptr[8], returns=None, traj=ptr[9], pitch=16, layout=_native.LAYOUTS["packed"], n=16, seed=1,
             lane0=8, t0=1, k_steps=0, flags=_native.POMDP_AUTO_RESET, stream=None)
    a.update(over)
    a["_keep"] = (keep, params, hist)
    return a


def _call(a):
    from gym_pomdp_amd import _native
    order = ("env", "params", "state", "b", "h", "prev_ob", "action", "ob", "reward", "done", "returns", "traj", "pitch", "layout", "n",
             "seed", "lane0", "t0", "k_steps", "flags", "stream")
    return _native.lib().pomdp_heuristic_collect(*[a[k] for k in order])


def test_bad_arguments_are_refused_before_any_launch():
    """k_steps == 0 is a no-op for arguments nothing is wrong with (no launch: no GPU needed); each single fault returns
    POMDP_E_BADARG — with k_steps = 64 too, where a call that got past the checks would launch."""
    from gym_pomdp_amd import _native
    lay = _native.LAYOUTS
    assert _call(_args()) == 0
    assert _call(_args(layout=lay["narrow"])) == 0
    assert _call(_args(n=0, k_steps=64)) == 0                            # an empty shard: nothing to launch either
    bad = [dict(traj=None), dict(pitch=15), dict(layout=lay["narrow"], pitch=18), dict(lane0=6), dict(layout=lay["columns"]),
           dict(layout=lay["blocked"]), dict(layout=4), dict(layout=-1), dict(k_steps=-1), dict(state=None), dict(prev_ob=None),
           dict(action=None), dict(ob=None), dict(reward=None), dict(done=None), dict(h=None), dict(params=None), dict(env=9),
           dict(n=-1), dict(n=1 << 32, pitch=1 << 33, lane0=4), dict(layout=lay["narrow"], pitch=1 << 31)]
    for over in bad:
        for k in (0, 64):
            assert _call(_args(**dict(dict(k_steps=k), **over))) == -1, (over, k)
    # everything NULL, as test_bad_arguments_are_rejected_without_a_gpu calls the other entry points
    assert _native.lib().pomdp_heuristic_collect(0, None, None, None, None, None, None, None, None, None, None, None, 16, 2, 16, 0, 0, 0, 4,
                                                 1, None) == -1
    r = _native.Returns(0.95, None, None, None)                          # `returns` given, its arrays missing
    assert _call(_args(returns=C.byref(r))) == -1


def test_python_side_checks_fire_before_the_device_is_touched():
    """collect_heuristic on an env object that was never set up: each check raises before anything of the env is used."""
    import gym_pomdp_amd as gpa
    e = object.__new__(gpa.TagEnv)
    hist = types.SimpleNamespace(prev_ob=object())
    e._has_reset = False
    with pytest.raises(AttributeError, match="before reset"):
        e.collect_heuristic(hist, 4)
    e._has_reset, e.lane_offset = True, 0
    with pytest.raises(ValueError, match="current observation"):
        e.collect_heuristic(types.SimpleNamespace(prev_ob=None), 4)
    for layout in ("columns", "blocked", "returns", None):
        with pytest.raises(ValueError, match="layout"):
            e.collect_heuristic(hist, 4, layout=layout)
    with pytest.raises(ValueError, match="steps"):
        e.collect_heuristic(hist, -1)
    e.lane_offset = 6
    with pytest.raises(ValueError, match="multiple of 4"):
        e.collect_heuristic(hist, 4)
