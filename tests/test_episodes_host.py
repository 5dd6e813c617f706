"""Host-side checks of the frozen-lane loops (ABI 15; no GPU needed): what the compiled kernels of episodes.hip look like, and the
ctypes mirror of pomdp_episode_args."""
import ctypes as C
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_episode_args_match_the_header_as_gcc_lays_it_out(tmp_path):
    """pomdp_episode_args against its ctypes mirror: sizeof and the offset of every field, from a program gcc compiles against
    the header itself (the method of test_host_logic's struct check, for the struct it does not list)."""
    from gym_pomdp_amd import _native as n
    pairs = {"pomdp_episode_args": n.EpisodeArgs, "pomdp_tape": n.Tape, "pomdp_return_stats": n.ReturnStats}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pomdp_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append('printf("POMDP_LAYOUT_RETURNS %d\\n", (int)POMDP_LAYOUT_RETURNS);')
    lines.append('printf("POMDP_ABI_VERSION %d\\n", (int)POMDP_ABI_VERSION);')
    lines.append('return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in pairs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    assert int(got["POMDP_LAYOUT_RETURNS"]) == n.POMDP_LAYOUT_RETURNS
    assert int(got["POMDP_ABI_VERSION"]) == n.ABI_VERSION == 15


def test_the_new_entry_points_are_declared_exported_and_bound():
    from gym_pomdp_amd import _native
    hdr = open(os.path.join(REPO, "include", "pomdp_hip.h")).read()
    for sym in ("pomdp_reset_where", "pomdp_finish_episodes"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in _native.SYMBOLS
    assert "episodes.hip" in _native.UNITS
    L = _native.lib()
    assert L.pomdp_finish_episodes(None, 0, 1, None) == -1
    assert L.pomdp_reset_where(0, None, None, None, None, None, 16, 0, 0, 0, None) == -1


def test_frozen_step_loops_never_wait_for_their_own_stores(tmp_path):
    """tools/check_loop_waits.py on episodes.hip: the synthetic-policy step loops hold no `s_waitcnt vmcnt` (a wait there would
    stall every step on the previous step's stores); a tape-driven loop waits once per step, for the row it asked for a step
    ahead.  Network's lane step reads its thresholds from the kernel arguments inside its per-lane draw loop, one more wait
    there, as in steps_kernel<NetworkEnv, 1, false>.  Every step loop runs the priority ladder (four s_setprio)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_loop_waits as clw
    res = clw.loop_waits(clw.assembly("episodes.hip", out_dir=str(tmp_path)))
    seen = 0
    for name, (waits, prio) in res.items():
        if not name.startswith("void pomdp::episodes_"):
            continue
        seen += 1
        assert prio == 4, (name, prio)
        taped = ", true>(" in name or "TapeQuad>(" in name
        allowed = (1 if taped else 0) + (1 if "NetworkEnv" in name else 0)
        assert len(waits) <= allowed, (name, waits)
        if "RockEnv" in name and not taped:
            assert waits == [], (name, waits)
    # eleven env types x three sinks x two policies (general loop) + four RockSample types x three sinks x two policies (quad loop)
    assert seen == 11 * 3 * 2 + 4 * 3 * 2, seen


def test_frozen_step_loops_keep_nothing_in_scratch_memory():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = kr.collect(units=["episodes.hip"])
    names = [r["kernel"] for r in rows]
    assert sum(1 for k in names if k.startswith("reset_where_kernel<")) == 11
    assert sum(1 for k in names if k.startswith("episodes_quad_kernel<")) == 24
    assert sum(1 for k in names if k.startswith("episodes_kernel<")) == 66
    bad = [(r["kernel"], r["scratch"]) for r in rows if r["scratch"] != "0"]
    assert not bad, bad
