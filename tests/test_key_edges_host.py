"""The top of the lane range at the C ABI, without a GPU: every entry point that draws random words refuses a lane range that
runs past 2^32 (the Philox counter's lane word would wrap onto the lanes of another shard) and accepts the range whose last lane
is 0xFFFFFFFF.  Every check runs on the host before anything is enqueued: the device pointers here are fake and never
dereferenced.  Entry points that have no step count (step, reset, reset_where, the stand-alone policy, rollout, plan) launch
whenever they accept a non-empty batch, so their acceptance of lane0 = 2^32 - n is shown on real buffers in
tests/test_gpu_key_edges.py; here they are shown to accept the same arguments with an empty batch at the top of the range."""
import ctypes as C

N = 1024
TOP = (1 << 32) - N                     # the last lane is 0xFFFFFFFF
PAST = TOP + 4                          # a multiple of 4 (no other check fires); lane0 + n = 2^32 + 4
SEED, T0 = 0x9E3779B97F4A7C15, (1 << 32) - 7
X = 1 << 40                             # a fake, 16-byte aligned "device" address
BADARG = -1                             # POMDP_E_BADARG (include/pomdp_hip.h: "n + lane0 > 2^32")
AUTO = 1                                # POMDP_AUTO_RESET


def _rock_params():
    from gym_pomdp_amd import _native
    p = _native.RockParams(size=7, num_rocks=8, start_x=0, start_y=3)
    for i in range(256):
        p.grid[i] = -1
    for i in range(32):
        p.thr[i] = 1 << 52
    return p


def _calls():
    """name -> f(n, lane0, k): the entry point on valid arguments with that lane range and step count"""
    from gym_pomdp_amd import _native
    L = _native.lib()
    params = _rock_params()
    p = C.byref(params)
    keep = [params]                      # the structs the closures point into
    tape = _native.Tape(actions=X, stride=N)
    stats = _native.ReturnStats(.95, X, X, N)
    bel = _native.RockBelief(*[X] * 6)
    hist = _native.HistoryPtrs(X, X, X, X, X, X, None, None, -1, 0)
    po = _native.PlanOut(q=X, visits=X, best=X, value=X, stride=13, reserved=0)
    keep += [tape, stats, bel, hist, po]
    packed, rets = _native.LAYOUTS["packed"], _native.POMDP_LAYOUT_RETURNS

    def collect(n, lane0, k):
        a = _native.CollectArgs(env=0, flags=AUTO, params=C.addressof(params), state=X, action=X, ob=X, reward=X, done=X, err=None,
                                n=n, pitch=N, seed=SEED, lane0=lane0, reserved=0)
        return L.pomdp_collect(C.byref(a), T0, k, None)

    def collect_traj(n, lane0, k):
        a = _native.TrajArgs(env=0, flags=AUTO, layout=packed, reserved=0, params=C.addressof(params), state=X, traj=X, err=None, n=n,
                             pitch=N, seed=SEED, lane0=lane0, reserved2=0)
        return L.pomdp_collect_traj(C.byref(a), T0, k, None)

    def finish(layout):
        def f(n, lane0, k):
            a = _native.EpisodeArgs(env=0, layout=layout, params=C.addressof(params), state=X, done=X, tape=None,
                                    traj=None if layout == rets else X, pitch=N, stats=C.addressof(stats) if layout == rets else None,
                                    err=None, n=n, seed=SEED, lane0=lane0, reserved=0)
            return L.pomdp_finish_episodes(C.byref(a), T0, k, None)
        return f

    def step_bound(n, lane0, k):
        a = _native.StepArgs(env=0, flags=AUTO, params=C.addressof(params), state=X, ob=X, reward=X, done=X, err=None, n=n, seed=SEED,
                             lane0=lane0, reserved=0)
        return L.pomdp_step(C.byref(a), X, T0, None)

    with_steps = {
        "pomdp_collect_synthetic": lambda n, l0, k: L.pomdp_collect_synthetic(0, p, X, X, X, X, X, None, n, SEED, l0, T0, k, N, AUTO, None),
        "pomdp_collect": collect,
        "pomdp_collect_layout": lambda n, l0, k: L.pomdp_collect_layout(0, p, X, X, None, n, SEED, l0, T0, k, N, packed, AUTO, None),
        "pomdp_collect_traj": collect_traj,
        "pomdp_collect_returns": lambda n, l0, k: L.pomdp_collect_returns(0, p, X, C.byref(stats), None, n, SEED, l0, T0, k, AUTO, None),
        "pomdp_collect_tape": lambda n, l0, k: L.pomdp_collect_tape(0, p, X, C.byref(tape), X, X, X, None, n, SEED, l0, T0, k, N, AUTO, None),
        "pomdp_collect_tape_layout": lambda n, l0, k: L.pomdp_collect_tape_layout(0, p, X, C.byref(tape), X, None, n, SEED, l0, T0, k, N,
                                                                                 packed, AUTO, None),
        "pomdp_collect_tape_returns": lambda n, l0, k: L.pomdp_collect_tape_returns(0, p, X, C.byref(tape), C.byref(stats), None, n, SEED,
                                                                                   l0, T0, k, AUTO, None),
        "pomdp_finish_episodes[packed]": finish(packed),
        "pomdp_finish_episodes[returns]": finish(rets),
        "pomdp_rollout_synthetic": lambda n, l0, k: L.pomdp_rollout_synthetic(0, p, X, X, X, X, X, None, n, SEED, SEED, l0, T0, k,
                                                                             AUTO | _native.POMDP_FUSE_STEPS, None),
        "pomdp_rollout_synthetic[other policy key]": lambda n, l0, k: L.pomdp_rollout_synthetic(0, p, X, X, X, X, X, None, n, SEED,
                                                                                               SEED ^ 1 << 32, l0, T0, k, AUTO, None),
        "pomdp_heuristic_steps": lambda n, l0, k: L.pomdp_heuristic_steps(0, p, X, C.byref(bel), C.byref(hist), X, X, X, X, X, None, n,
                                                                         SEED, l0, T0, k, AUTO, None),
    }
    # no step count: a non-empty batch that is accepted is launched (k is ignored)
    launch_only = {
        "pomdp_step": step_bound,
        "pomdp_rock_step": lambda n, l0, k: L.pomdp_rock_step(p, X, X, X, X, X, None, n, SEED, l0, T0, AUTO, None),
        "pomdp_rock_reset": lambda n, l0, k: L.pomdp_rock_reset(p, X, X, n, SEED, l0, T0, None),
        "pomdp_reset_where": lambda n, l0, k: L.pomdp_reset_where(0, p, X, X, X, X, n, SEED, l0, T0, None),
        "pomdp_synthetic_actions": lambda n, l0, k: L.pomdp_synthetic_actions(X, n, SEED, l0, T0, 13, None),
        "pomdp_pick_actions": lambda n, l0, k: L.pomdp_pick_actions(X, X, 13, X, n, SEED, l0, T0, None),
        "pomdp_rollout": lambda n, l0, k: L.pomdp_rollout(0, p, X, n // 64, 64, 16, .95, 0, SEED, l0, T0, X, X, X, X, X, None),
        "pomdp_plan": lambda n, l0, k: L.pomdp_plan(0, p, X, n // 64, 64, 16, .95, 0, SEED, l0, T0, X, X, C.byref(po), None),
    }
    return with_steps, launch_only, keep


def test_a_lane_range_past_2_32_is_refused_by_every_drawing_entry_point():
    with_steps, launch_only, _keep = _calls()
    for name, f in list(with_steps.items()) + list(launch_only.items()):
        assert f(N, PAST, 20) == BADARG, name


def test_the_range_that_ends_at_lane_0xffffffff_is_accepted():
    """lane0 = 2^32 - n exactly, with no steps to run: 0, and nothing is launched.  The same calls one quad further up are the
    refusals above, so it is the range check that tells them apart."""
    with_steps, _, _keep = _calls()
    for name, f in with_steps.items():
        assert f(N, TOP, 0) == 0, name
        assert f(N, PAST, 0) == BADARG, name


def test_entry_points_without_a_step_count_accept_an_empty_batch_at_the_top():
    """n = 0 at lane0 = 0xFFFFFFFC: the other arguments of the refused calls above are valid (0, nothing launched), so those
    refusals are the range check's.  A non-empty batch that ends at lane 0xFFFFFFFF runs in tests/test_gpu_key_edges.py."""
    _, launch_only, _keep = _calls()
    for name, f in launch_only.items():
        assert f(0, 0xFFFFFFFC, 0) == 0, name
        assert f(N, PAST, 0) == BADARG, name


def test_the_host_mirror_passes_the_edge_coordinates_unchanged():
    """The ctypes signatures carry a call counter above 2^63 and a seed with its top bit set as the unsigned 64-bit values they
    are (a signed declaration would raise or wrap), and lane0 = 2^32 - 4 as an unsigned 32-bit one."""
    from gym_pomdp_amd import _native
    L = _native.lib()
    u64_at = {"pomdp_collect": (1,), "pomdp_collect_traj": (1,), "pomdp_finish_episodes": (1,), "pomdp_step": (2,),
              "pomdp_collect_synthetic": (9, 11), "pomdp_collect_layout": (6, 8), "pomdp_collect_returns": (6, 8),
              "pomdp_collect_tape": (9, 11), "pomdp_collect_tape_layout": (7, 9), "pomdp_collect_tape_returns": (7, 9),
              "pomdp_rollout_synthetic": (9, 10, 12), "pomdp_heuristic_steps": (12, 14), "pomdp_reset_where": (7, 9),
              "pomdp_synthetic_actions": (2, 4), "pomdp_rollout": (8, 10), "pomdp_plan": (8, 10), "pomdp_rock_reset": (4, 6),
              "pomdp_rock_step": (8, 10)}
    for name, idx in u64_at.items():
        at = getattr(L, name).argtypes
        assert all(at[i] is C.c_uint64 for i in idx), name
    t0 = 0xFFFFFFFEFFFFFFF9
    assert C.c_uint64(t0).value == t0 and C.c_uint64((1 << 64) - 1).value == (1 << 64) - 1
    for struct in (_native.StepArgs, _native.CollectArgs, _native.TrajArgs, _native.EpisodeArgs):
        f = dict(struct._fields_)
        assert f["seed"] is C.c_uint64 and f["lane0"] is C.c_uint32, struct
        s = struct(seed=(1 << 64) - 1, lane0=0xFFFFFFFC)
        assert s.seed == (1 << 64) - 1 and s.lane0 == 0xFFFFFFFC
