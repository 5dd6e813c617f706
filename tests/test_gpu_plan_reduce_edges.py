"""pomdp_plan_reduce called through the C ABI on what no env's rollouts give it: action counts from 1 to the limit of 255,
simulation counts around the 64-simulation chunk and the 1024-simulation tile, returns spread over thirteen decades, exact
ties, -0.0, infinities, NaN, roots nothing visited, and first actions beyond the action count — against the oracle, q and
value bit for bit (test_plan_reduce_host.py pins the oracle to the header's words and shows the inputs tell the orders apart)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_reduce_restatement as prr  # noqa: E402
from test_plan_reduce_host import check_equal, check_special  # noqa: E402

pytestmark = pytest.mark.gpu
Q_FILL, V_FILL, B_FILL = 7.5, -3, -77


def plan_reduce(ret, fa, R, S, A, stride, with_value):
    """-> (what the kernel wrote in columns < A, as oracle_lib.plan_reduce returns it; value None without a value
    pointer), after checking that the columns past A still hold their fill"""
    from gym_pomdp_amd import _native
    d_ret, d_fa = torch.as_tensor(ret, device="cuda"), torch.as_tensor(fa, device="cuda")
    q = torch.full((R, stride), Q_FILL, dtype=torch.float64, device="cuda")
    visits = torch.full((R, stride), V_FILL, dtype=torch.int32, device="cuda")
    best = torch.full((R,), B_FILL, dtype=torch.int32, device="cuda")
    value = torch.full((R,), Q_FILL, dtype=torch.float64, device="cuda")
    po = _native.PlanOut(q=q.data_ptr(), visits=visits.data_ptr(), best=best.data_ptr(), value=value.data_ptr() if with_value else None,
                         stride=stride, reserved=0)
    assert _native.lib().pomdp_plan_reduce(d_ret.data_ptr(), d_fa.data_ptr(), R, S, A, C.byref(po), None) == 0
    torch.cuda.synchronize()
    q, visits, value = q.cpu().numpy(), visits.cpu().numpy(), value.cpu().numpy()
    assert (q[:, A:] == Q_FILL).all() and (visits[:, A:] == V_FILL).all()
    if not with_value:
        assert (value == Q_FILL).all()
    return dict(q=np.ascontiguousarray(q[:, :A]), visits=visits[:, :A], best=best.cpu().numpy(), value=value)


@pytest.mark.parametrize("S,A", prr.SHAPES, ids=["S%d-A%d" % c for c in prr.SHAPES])
def test_plan_reduce_at_the_edges_of_its_shapes(oracle_lib, S, A):
    """stride = A and A + 3, with and without a value pointer, alternating over the shapes (both strides at A = 255)"""
    i = prr.SHAPES.index((S, A))
    ret, fa = prr.shape_inputs(S, A)
    want = oracle_lib.plan_reduce(ret, fa, prr.ROOTS, S, A)
    calls = [(A + 3 * (i % 2), i % 3 != 0)]
    if A in (1, 255):
        calls.append((A + 3 * ((i + 1) % 2), i % 3 == 0))
    for stride, with_value in calls:
        got = plan_reduce(ret, fa, prr.ROOTS, S, A, stride, with_value)
        if not with_value:
            got["value"] = want["value"]
        check_equal(got, want, (S, A, stride, with_value))


def test_plan_reduce_on_the_special_roots(oracle_lib):
    ret, fa = prr.special_roots()
    R = len(prr.SPECIAL)
    want = oracle_lib.plan_reduce(ret, fa, R, prr.SPECIAL_S, prr.SPECIAL_A)
    got = plan_reduce(ret, fa, R, prr.SPECIAL_S, prr.SPECIAL_A, prr.SPECIAL_A + 3, True)
    check_equal(got, want, ("special",))
    check_special(got)


@pytest.mark.parametrize("A", [4, 255])
def test_first_actions_beyond_the_action_count_count_for_no_action(oracle_lib, A):
    ret, fa, counted = prr.out_of_range_inputs(A)
    want = oracle_lib.plan_reduce(ret, fa, 1, len(fa), A)
    got = plan_reduce(ret, fa, 1, len(fa), A, A, True)
    check_equal(got, want, ("out of range", A))
    assert int(got["visits"].sum()) == counted
