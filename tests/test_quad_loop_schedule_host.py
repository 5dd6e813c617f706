"""How RockSample's quad loops are SCHEDULED around their table reads (static, no GPU: the compiled assembly of
csrc/fused_rock.hip and csrc/fused_stochrock.hip through tools/check_loop_waits.py).

The one-state-word lane step reads the table entries of all four lanes of a thread and waits once.  A wave that has nothing of
its own to issue between the last read and that wait sits through the whole LDS round trip; the synthetic policy's Philox block
(15 v_mad_u64_u32 + 15 v_bitop3_b32, then four v_mul_hi_u32) does not depend on the step's state and belongs there
(fused_impl.hip.h: UNDER_READS).  Left to itself the compiler sinks the block below the records — the count asserted here was 0
in every one of these kernels."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINKS = ("pomdp::ColumnsT<true>", "pomdp::Blocked", "pomdp::Packed", "pomdp::Narrow", "pomdp::Returns<pomdp::RockEnv<1, false> >")
# (unit, kernel, the table read of its form: RecWide's 16-byte entries, RecRot's 8-byte ones)
CASES = [("fused_rock.hip", "steps_quad_kernel<pomdp::RockEnv<1, false>, %s, pomdp::SyntheticQuad, 4>" % s, "ds_read_b128") for s in SINKS]
CASES.append(("fused_stochrock.hip", "steps_quad_kernel<pomdp::RockEnv<1, true>, pomdp::Packed, pomdp::SyntheticQuad, 4>", "ds_read_b128"))
CASES.append(("fused_rock.hip", "steps_quad_popc_kernel<pomdp::RockEnv<1, false>, pomdp::Packed, pomdp::SyntheticQuad, 4>", "ds_read_b64"))


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_loop_waits as clw
    out = str(tmp_path_factory.mktemp("asm"))
    return {u: clw.kernel_bodies(clw.assembly(u, out_dir=out)) for u in sorted({c[0] for c in CASES})}


@pytest.mark.parametrize("unit,kernel,read", CASES, ids=[c[1].replace("pomdp::", "") for c in CASES])
def test_policy_block_issues_under_the_table_reads(bodies, unit, kernel, read):
    import check_loop_waits as clw
    match = [b for name, b in bodies[unit].items() if name.split("(")[0].replace("void ", "").replace("pomdp::steps", "steps", 1).strip() == kernel]
    assert len(match) == 1, (kernel, len(match))
    groups = clw.under_reads(match[0], read)
    # the step loop's group is the one of FOUR reads, a thread's four lanes (a loop's other reads of that width are the tie
    # paths', one at a time)
    quad = [g for g in groups if g[0] == 4]
    assert len(quad) == 1, (kernel, groups)
    reads, philox, branches = quad[0]
    print(kernel, "-> reads", reads, "Philox instructions between the last of them and the wait", philox, "branches", branches)
    assert philox >= 28, (kernel, groups)
    assert branches == 0, (kernel, groups)          # the block is straight-line code: nothing leaves between the reads and the wait


def test_no_quad_loop_pays_for_the_schedule_with_a_wave():
    """The block under the reads keeps its four actions live across the records: four more registers (the headline kernel 78 ->
    82).  Registers are free only up to the next occupancy step, so every one-state-word quad loop under the synthetic policy is held to the waves per
    SIMD it had before (tools/kernel_resources.py: hipcc's own remark) — five on the 16-byte table (27 KB of LDS), four on
    the 8-byte one (35 KB) and in the returns sinks (their 120-128 registers) — the 4-byte and column sinks on the 16-byte
    table stay within the 96 registers five waves allow, and nothing spills.  StochasticRock's returns and column sinks would
    have lost a wave (126 -> 130, 94 -> 98): under_reads_fits (fused_impl.hip.h) leaves them out."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    rows = [r for r in kr.collect(["fused_rock.hip", "fused_stochrock.hip"]) 
            if r["kernel"].startswith("steps_quad") and "RockEnv<1, " in r["kernel"] and "SyntheticQuad" in r["kernel"]]
    assert len(rows) == 2 * 14, len(rows)              # per env: (popc + wide) x (five sinks + the two half-quad forms)
    for r in rows:
        k, returns = r["kernel"], "Returns<" in r["kernel"]
        want = 4 if returns or k.startswith("steps_quad_popc_kernel<") else 5
        print(r["vgpr"], r["occupancy"], k)
        assert int(r["occupancy"]) == want and r["scratch"] == "0", r
        assert int(r["vgpr"]) <= (128 if returns else 96 if want == 5 else 104), r
