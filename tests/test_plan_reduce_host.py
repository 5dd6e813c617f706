"""pomdp_plan_reduce's stated order without a GPU: the oracle's reduction (what test_gpu_plan_reduce_edges.py holds the
kernel to) equals a Python-float restatement of the header's words bit for bit on the edge shapes and the special roots,
and the inputs tell that order from the others a reduction might take."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_reduce_restatement as prr  # noqa: E402


def same_bits(x, y):
    """float64 bit for bit; any NaN equals any NaN"""
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    return bool(((x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))).all())


def check_equal(got, want, ctx):
    for k in ("q", "value"):
        assert same_bits(got[k], want[k]), ctx + (k,)
    for k in ("visits", "best"):
        assert np.array_equal(got[k], want[k]), ctx + (k,)


def check_special(out):
    """the values the special roots must give (root order: prr.SPECIAL)"""
    q, visits, best, value = out["q"], out["visits"], out["best"], out["value"]
    assert best[0] == 1 and value[0] == 2.5 and q[0, 1] == 2.5 and q[0, 3] == 2.5 and visits[0, 2] == 0      # the first of a tie
    assert best[1] == 2 and value[1] == -7.0 and visits[1].tolist() == [0, 0, 44, 0]                           # beats nothing's 0.0
    assert best[2] == 1 and np.isnan(value[2]) and np.isnan(q[2, 1]) and q[2, 2] == 5.0                        # nothing is > NaN
    assert best[3] == 0 and value[3] == 1.0 and np.isnan(q[3, 2]) and q[3, 3] == .5                            # NaN is > nothing
    assert (q[4].view(np.uint64) == 0).all() and best[4] == 0 and value[4:5].view(np.uint64)[0] == 0           # +0.0, sign bit clear
    assert np.isnan(q[5, 1]) and np.isfinite(q[5, [0, 2, 3]]).all()                                            # inf + -inf
    assert best[6] == -1 and value[6] == 0.0 and (visits[6] == 0).all() and (q[6].view(np.uint64) == 0).all()


@pytest.mark.parametrize("S,A", prr.SHAPES, ids=["S%d-A%d" % c for c in prr.SHAPES])
def test_oracle_equals_the_stated_order_and_no_other(oracle_lib, S, A):
    ret, fa = prr.shape_inputs(S, A)
    want = oracle_lib.plan_reduce(ret, fa, prr.ROOTS, S, A)
    check_equal(prr.reduce(ret, fa, prr.ROOTS, S, A), want, (S, A))
    assert (want["visits"].sum(axis=1) == (fa.reshape(prr.ROOTS, S) >= 0).sum(axis=1)).all()
    if S >= 1023:
        for order in prr.ORDERS[1:]:
            other = prr.reduce(ret, fa, prr.ROOTS, S, A, order)
            assert np.array_equal(other["visits"], want["visits"])
            assert (other["q"].view(np.uint64) != want["q"].view(np.uint64)).any(), (S, A, order)


def test_oracle_on_the_special_roots_and_out_of_range_first_actions(oracle_lib):
    ret, fa = prr.special_roots()
    R = len(prr.SPECIAL)
    want = oracle_lib.plan_reduce(ret, fa, R, prr.SPECIAL_S, prr.SPECIAL_A)
    check_equal(prr.reduce(ret, fa, R, prr.SPECIAL_S, prr.SPECIAL_A), want, ("special",))
    check_special(want)
    for A in (4, 255):
        ret, fa, counted = prr.out_of_range_inputs(A)
        want = oracle_lib.plan_reduce(ret, fa, 1, len(fa), A)
        check_equal(prr.reduce(ret, fa, 1, len(fa), A), want, ("out of range", A))
        assert int(want["visits"].sum()) == counted
