"""Edge values on the CPU implementation (oracle/) against the exact reference of tests/edge_cases.py: every column family, the
program templates over a few seeds and the fixed tuple shapes at every size, and a changed column's contents.  This pins the
evaluator and the cases, as test_code_space_comparison_cases_on_the_cpu_implementation does for the code-space cases."""
import math

import numpy as np
import pytest

import edge_cases as E
from sdqlpy_amd import abi as A


@pytest.fixture(scope="module")
def cpu_ctx(oracle_lib):
    ctx = oracle_lib.context(threads=4)
    yield ctx
    ctx.close()


def test_edge_values_on_the_cpu_implementation(cpu_ctx):
    chk = E.all_cases(cpu_ctx, seeds=(1, 2))
    assert chk.checks > 100000
    assert sum(1 for r in chk.records if r[1] == 1) > 1000            # single-row groups, compared bit for bit


def test_evaluator_follows_c():
    """The evaluator's own semantics on hand-picked rows: truncating division, I2F rounding, NaN comparisons, -0.0 == 0.0,
    CHAR past the text, the INT64_MIN row flagged only when it is not gated out."""
    class Col:
        pass
    xi, xf, xt = Col(), Col(), Col()
    ints = np.array([-7, 7, (1 << 53) + 1, E.I64_LO], np.int64)
    flts = np.array([math.nan, -0.0, 0.0, 1.0])
    host = {id(xi): ints, id(xf): flts, id(xt): np.array(["ab", "", "\U0001F600c", "abcd"], "<U4")}
    P = A.Program()
    i = P.op(A.X_COL, A.T_I64, col=xi); f = P.op(A.X_COL, A.T_F64, col=xf)
    small = P.op(A.X_GT, A.T_BOOL, a=i, b=P.op(A.X_CONST, A.T_I64, imm_i=E.I64_LO))
    P.gates = [small]
    zero = P.op(A.X_CONST, A.T_F64, imm_f=0.0)
    P.vals = [P.op(A.X_DIVI, A.T_I64, a=i, imm_i=2), P.op(A.X_MODI, A.T_I64, a=i, imm_i=2), P.op(A.X_I2F, A.T_F64, a=i),
              P.op(A.X_EQ, A.T_BOOL, a=f, b=zero), P.op(A.X_NE, A.T_BOOL, a=f, b=f), P.op(A.X_CHAR, A.T_I64, col=xt, aux=1),
              P.op(A.X_NEG, A.T_I64, a=i)]
    ev = E.evaluate(P, 4, host)
    assert ev.passing.tolist() == [True, True, True, False]
    assert not ev.flagged.any()                                      # -INT64_MIN only on the row the gate drops
    assert ev.vals[0].tolist()[:2] == [-3, 3] and ev.vals[1].tolist()[:2] == [-1, 1]
    assert ev.vals[2][2] == float(1 << 53)                           # 2^53 + 1 rounds to even
    assert ev.vals[3].tolist() == [False, True, True, False] and ev.vals[4].tolist() == [True, False, False, False]
    assert ev.vals[5].tolist() == [ord("b"), 0, ord("c"), ord("b")]
    P.gates = []
    assert E.evaluate(P, 4, host).flagged.tolist() == [False, False, False, True]


def test_sum_rules_bite():
    """The comparison rules reject what they are there to reject."""
    chk = E.Checker()
    chk.sum(0.1 * (1.0 - 0.3), [0.1 * (1.0 - 0.3)], "one row")
    with pytest.raises(AssertionError):
        chk.sum(math.nextafter(0.07, 1.0), [0.07], "one row, one ulp off")
    with pytest.raises(AssertionError):
        chk.sum(-0.0, [-0.0, -0.0], "zeros sum to +0.0")
    with pytest.raises(AssertionError):
        chk.sum(0.0, [2.0 ** -1074, 2.0 ** -1073], "flushed subnormal values")
    with pytest.raises(AssertionError):
        chk.sum(math.inf, [math.inf, -math.inf], "both infinities")
    with pytest.raises(AssertionError):
        chk.sum(0.6 + 4 * math.ulp(0.6), [0.1, 0.2, 0.3], "three rows, past the bound")
    chk.sum(0.1 + 0.2 + 0.3, [0.3, 0.2, 0.1], "three rows, another order")
    chk.sum(0.0, [1e16, 1.0, -1e16, 1.0], "heavy cancellation within (m-1) u sum|x|")
