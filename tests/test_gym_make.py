"""The plugin boundary: `gym.make("Rock-v0")` (gym_pomdp/__init__.py:7-46, readme.md:18-24) against stand-ins that do what
real gym 0.21 and real gymnasium do to the object an entry point builds (oracle/ref_harness/stubs: `EnvSpec.make` sets
`env.unwrapped.spec`, wraps in OrderEnforcing, refuses to re-register an id; stubs_gymnasium: the `isinstance(env,
gymnasium.Env)` check, PassiveEnvChecker, the new reset / step api).  Neither package is installed in this image, and the
product picks its base class at import, so every case runs in a child interpreter with the stand-in on its path.

CPU: everything up to the point the env needs the GPU.  `-m gpu`: gym.make(...) -> reset -> step == gym_pomdp_amd.make(...)."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

GYM_STUB = os.path.join(REPO, "oracle", "ref_harness", "stubs")
GYMNASIUM_STUB = os.path.join(REPO, "oracle", "ref_harness", "stubs_gymnasium")


def run_child(code, *paths, timeout=600):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=os.pathsep.join(list(paths) + [REPO]))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    assert out.returncode == 0 and "child ok" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    return out.stdout


def test_old_gym_make_reaches_the_batched_class():
    run_child("""
import gym, torch
import gym_pomdp_amd as gpa
from gym_pomdp_amd import compat, spaces
specs = gym.envs.registration.registry.env_specs
want = {"Rock-v0": "RockEnv", "Tag-v0": "TagEnv", "Battleship-v0": "BattleShipEnv", "Tiger-v0": "TigerEnv",
        "Network-v0": "NetworkEnv", "StochasticRock-v0": "StochasticRockEnv"}
for env_id, cls in want.items():
    assert specs[env_id].entry_point == "gym_pomdp_amd.envs:" + cls, specs[env_id].entry_point
    assert issubclass(getattr(gpa, cls), gym.Env)                     # what gym's wrappers and checkers test
assert compat.EnvBase is gym.Env and spaces.Discrete is gym.spaces.Discrete
assert gpa.RockEnv.spec is None and isinstance(gpa.RockEnv.unwrapped, property) and isinstance(gpa.RockEnv.np_random, property)
assert gpa.RockEnv.metadata["render.modes"] == ["ansi"] and gpa.RockEnv.metadata["render_modes"] == ["ansi"]
# a second registration pass finds the ids and leaves them alone; the registry itself refuses (gym 0.21)
assert gpa._register_with_gym() == {"gym": []}
try:
    gym.register(id="Rock-v0", entry_point="x:y")
    raise SystemExit("re-registration went through")
except gym.error.Error:
    pass
if not torch.cuda.is_available():
    try:
        gym.make("Rock-v0", batch_size=4)
        raise SystemExit("built an env without a GPU")
    except RuntimeError as e:                                          # the class's own constructor spoke: no CPU fallback
        assert "no GPU" in str(e), e
print("child ok")
""", GYM_STUB)


def test_what_gym_make_touches_exists_on_the_env_object():
    """EnvSpec.make does `env.unwrapped.spec = spec` and wraps; the wrappers reach everything else by attribute.  Run on an
    instance whose constructor skipped the GPU part."""
    run_child("""
import gym
import gym_pomdp_amd as gpa
class Shell(gpa.RockEnv):
    def __init__(self, **kw):
        self._seed = 11
        self.kw = kw
gym.register(id="Shell-v0", entry_point=Shell, kwargs={"a": 1})
env = gym.make("Shell-v0", b=2)
inner = env.unwrapped
assert type(env).__name__ == "OrderEnforcing" and type(inner) is Shell and inner.kw == {"a": 1, "b": 2}
assert inner.spec.id == "Shell-v0" and env.spec is inner.spec and Shell.spec is None
assert inner.unwrapped is inner and env.metadata["render_modes"] == ["ansi"] and env.render_mode is None
r = inner.np_random
assert r is inner.np_random and int(r.randint(1 << 30)) == int(__import__("numpy").random.RandomState(11).randint(1 << 30))
try:
    env.step(0)
    raise SystemExit("step before reset went through the wrapper")
except AssertionError:
    pass
print("child ok")
""", GYM_STUB)


# A stand-in for the reference package as gym sees it: a `gym_pomdp` whose import registers the ids this package registers too,
# each to a class of its own modules (gym_pomdp/__init__.py, gym_pomdp/envs/*.py of d3sm0/gym_pomdp)
REFERENCE_IDS = {"Tiger-v0": ("tiger", "TigerEnv"), "Tag-v0": ("tag", "TagEnv"), "Battleship-v0": ("battleship", "BattleShipEnv"),
                 "Rock-v0": ("rock", "RockEnv"), "StochasticRock-v0": ("rock", "StochasticRockEnv"), "Network-v0": ("network", "NetworkEnv")}


def reference_stand_in(root):
    pkg = root / "gym_pomdp"
    (pkg / "envs").mkdir(parents=True)
    (pkg / "__init__.py").write_text("from gym.envs.registration import register\n" + "".join(
        "register(id=%r, entry_point=%r)\n" % (i, "gym_pomdp.envs:" + c) for i, (_, c) in REFERENCE_IDS.items()))
    mods = {}
    for m, c in REFERENCE_IDS.values():
        mods.setdefault(m, []).append(c)
    for m, classes in mods.items():
        (pkg / "envs" / (m + ".py")).write_text("import gym\n" + "".join("class %s(gym.Env):\n    pass\n" % c for c in classes))
    (pkg / "envs" / "__init__.py").write_text("".join("from gym_pomdp.envs.%s import %s\n" % (m, c) for m, c in REFERENCE_IDS.values()))
    return str(root)


def test_the_reference_registered_first_keeps_its_ids(tmp_path):
    """Both packages imported in one process (the parity harness does that): the reference's registrations stay, ours are
    skipped without an exception; any error other than gym's own re-registration error propagates."""
    run_child("""
import gym, gym_pomdp
import gym_pomdp_amd as gpa
from gym_pomdp_amd import compat
specs = gym.envs.registration.registry.env_specs
assert specs["Rock-v0"].entry_point == "gym_pomdp.envs:RockEnv"
assert type(gym.make("Tag-v0").unwrapped).__module__ == "gym_pomdp.envs.tag"
# ids the pre-check cannot see: the registry's own error is swallowed, nothing else
compat._registered_ids = lambda reg: set()
assert compat.register_ids(gpa.registry) == {"gym": []}
reg = gym.envs.registration
def broken(id, **kw):
    raise ValueError("not a re-registration")
orig, reg.register = reg.register, broken
try:
    compat.register_ids(gpa.registry)
    raise SystemExit("a foreign exception was swallowed")
except ValueError:
    pass
reg.register = orig
print("child ok")
""", GYM_STUB, reference_stand_in(tmp_path))


def test_gymnasium_make_gets_a_gymnasium_env():
    run_child("""
import gymnasium, torch
import gym_pomdp_amd as gpa
from gym_pomdp_amd import compat
assert compat.gym is None and compat.EnvBase is object and issubclass(compat.GymnasiumEnv, gymnasium.Env)
assert sorted(gymnasium.registry) == sorted(gpa.registry)
assert all(callable(s.entry_point) for s in gymnasium.registry.values())
# the old-api class itself is NOT a gymnasium.Env: handing it to gymnasium.make is the TypeError the adapter exists for
gymnasium.register(id="Raw-v0", entry_point=lambda **kw: object.__new__(gpa.TigerEnv))
try:
    gymnasium.make("Raw-v0")
    raise SystemExit("gymnasium.make accepted a non-gymnasium env")
except TypeError:
    pass
# the adapter, driven through gymnasium.make's wrappers, around an old-api object
class Old(object):
    def __init__(self):
        self.action_space = gpa.spaces.Discrete(3); self.observation_space = gpa.spaces.Discrete(3)
        self.reward_range = (-20, 10); self.state = [0]; self.seeds = []; self.t = 0
    def seed(self, s=None): self.seeds.append(s)
    def reset(self): self.t = 0; return 2
    def step(self, a): self.t += 1; return a, -1, self.t == 3, {"state": self.state}
    def render(self): return "r"
    def close(self): self.closed = True
    extra = "forwarded"
gymnasium.register(id="Old-v0", entry_point=lambda **kw: compat.GymnasiumEnv(Old()))
env = gymnasium.make("Old-v0")
assert isinstance(env.unwrapped, gymnasium.Env) and env.unwrapped.spec.id == "Old-v0"
assert isinstance(env.action_space, gymnasium.spaces.Space) and env.action_space.n == 3
try:
    env.step(0)
    raise SystemExit("step before reset")
except gymnasium.error.ResetNeeded:
    pass
ob, info = env.reset(seed=5, options={"x": 1})
assert ob == 2 and info == {"state": [0]} and env.unwrapped.env.seeds == [5]
ob, info = env.reset()
assert env.unwrapped.env.seeds == [5]                                 # no seed given: seed() is not called
assert env.step(1) == (1, -1, False, False, {"state": [0]})
env.step(0)
assert env.step(2) == (2, -1, True, False, {"state": [0]})
assert env.unwrapped.extra == "forwarded" and env.render() == "r"
env.close(); assert env.unwrapped.env.closed
if not torch.cuda.is_available():
    try:
        gymnasium.make("Rock-v0", batch_size=4)
        raise SystemExit("built an env without a GPU")
    except RuntimeError as e:
        assert "no GPU" in str(e), e
print("child ok")
""", GYMNASIUM_STUB)


def test_without_any_gym_the_classes_stand_alone():
    run_child("""
import sys
assert "gym" not in sys.modules and "gymnasium" not in sys.modules
import gym_pomdp_amd as gpa
from gym_pomdp_amd import compat
assert compat.gym is None and compat.gymnasium is None and compat.EnvBase is object and compat.GymnasiumEnv is None
assert gpa._register_with_gym() == {} and gpa.spaces.Discrete is gpa.spaces._Discrete
assert gpa.RockEnv.spec is None and isinstance(gpa.RockEnv.unwrapped, property)
print("child ok")
""")


# ---------------------------------------------------------------------------------------------------------------------
GPU_OLD = """
import gym, torch
import gym_pomdp_amd as gpa
def same(a, b):
    return bool((a == b).all()) if isinstance(a, torch.Tensor) else a == b
for env_id, kw in (("Rock-v0", {}), ("Tag-v0", {}), ("Battleship-v0", {}), ("Tiger-v0", {}), ("Network-v0", {}),
                   ("StochasticRock-v0", {}), ("Rock-v0", dict(board_size=15, num_rocks=15))):
    for n in (1, 4096):
        e = gym.make(env_id, batch_size=n, seed=5, auto_reset=True, **kw)
        d = gpa.make(env_id, batch_size=n, seed=5, auto_reset=True, **kw)
        u = e.unwrapped
        assert type(e).__name__ == "OrderEnforcing" and type(u) is type(d) and u.spec.id == env_id
        assert u.spec._kwargs["batch_size"] == n and e.action_space == d.action_space
        assert isinstance(e.action_space, gym.spaces.Space)
        assert same(e.reset(), d.reset())
        for t in range(12):
            a = d.synthetic_actions() if n > 1 else int(d.synthetic_actions().item())
            got, want = e.step(a), d.step(a)
            assert all(same(g, w) for g, w in zip(got[:3], want[:3])), (env_id, n, t)
            assert same(got[3]["state"], want[3]["state"])
        assert same(e.state, d.state)                                  # batch extras through the wrapper
# the reference's own idiom: gym.make(id) with no arguments, python scalars, reset() when done (readme.md:18-24)
env = gym.make("Tiger-v0")
env.seed(3)
ob = env.reset()
assert ob == 2 and env.unwrapped.batch_size == 1
steps = 0
for t in range(50):
    ob, rw, done, info = env.step(env.action_space.sample())
    assert isinstance(ob, int) and isinstance(done, bool) and rw in (-1, -20, 10)
    steps += 1
    if done:
        env.reset()
# gym 0.22-0.25's wrappers pass reset(seed=, return_info=) through
e = gym.make("Tag-v0", batch_size=64, seed=1)
d = gpa.make("Tag-v0", batch_size=64, seed=9)
ob, info = e.reset(seed=9, return_info=True)
assert same(ob, d.reset()) and same(info["state"], d.state)
print("child ok")
"""

GPU_NEW = """
import gymnasium, torch
import gym_pomdp_amd as gpa
def same(a, b):
    return bool((a == b).all()) if isinstance(a, torch.Tensor) else a == b
for env_id in ("Rock-v0", "Tag-v0", "Battleship-v0", "Tiger-v0", "Network-v0"):
    for n in (1, 2048):
        e = gymnasium.make(env_id, batch_size=n, seed=1, auto_reset=True)
        d = gpa.make(env_id, batch_size=n, seed=7, auto_reset=True)
        u = e.unwrapped
        assert isinstance(u, gymnasium.Env) and type(u.env) is type(d) and u.spec.id == env_id
        assert isinstance(e.action_space, gymnasium.spaces.Space) and e.action_space.n == d.action_space.n
        ob, info = e.reset(seed=7)
        assert same(ob, d.reset()) and same(info["state"], d.state)
        for t in range(12):
            a = d.synthetic_actions() if n > 1 else int(d.synthetic_actions().item())
            ob, rw, term, trunc, info = e.step(a)
            want = d.step(a)
            assert same(ob, want[0]) and same(rw, want[1]) and same(term, want[2]), (env_id, n, t)
            assert (trunc is False) if n == 1 else (trunc.dtype == torch.bool and not bool(trunc.any()))
        assert same(u.state, d.state)
tr = gymnasium.make("Rock-v0", batch_size=4096, seed=2).unwrapped.collect_synthetic
print("child ok")
"""


@pytest.mark.gpu
def test_old_gym_make_equals_the_package_make_on_the_gpu():
    run_child(GPU_OLD, GYM_STUB)


@pytest.mark.gpu
def test_gymnasium_make_equals_the_package_make_on_the_gpu():
    run_child(GPU_NEW, GYMNASIUM_STUB)
