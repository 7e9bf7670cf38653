"""The bounds of tests/_qn_path_truth.py can tell a wrong shift apart: for every (state, mask, shift list) of the
dense-truth cases of tests/test_gpu_qn_path.py with a free row, the reference at mu (1 + 1e-6) lies OUTSIDE what the GPU
test allows around the reference at mu.  A condition on the inputs, not a measurement: nothing of the library runs
here, so these tests pass wherever the helper files are -- they say that the GPU tests' inputs are fit for their purpose.
  fp64 states, every shift: outside the Truth bound in at least one entry of the solve, for log det and for ||x||^2.
  REAL32 states: their Truth bounds carry the 2^-24 rounding of the imported middle matrix, which enters through the
  pairs' part of Sigma; against the diagonal part that falls off like theta / mu.  At the shifts of
  _qn_path_truth.MU32_SEES and above -- every REAL32 list has some -- a shift 1e-6 off is outside the state's own
  REAL32 bound in at least one entry of the solve and for ||x||^2, asserted here as for fp64.  At the smaller shifts
  of those lists it is not (the test prints by how much): they are there for the pairs' part, not for the shift.  Log det
  is held at EVERY shift by the comparison with the qn_shift route that the GPU test makes, within twice the bounds of
  _qn_path_truth.route_truth (the allowance is common to both routes and drops out of their difference).
Masks with no free row have nothing to tell apart (the GPU test asserts exact zeros there)."""
import numpy as np
import pytest

import _qn_path_truth as pt

CASES = [c for c in pt.CASES if c[1] != "all"]


def _v(n):
    return np.random.default_rng(4242 + n).standard_normal(n)


@pytest.mark.parametrize("case", CASES, ids=pt.case_id)
def test_a_wrong_shift_is_outside_the_bounds(case, oracle_built):
    state, mask, k, _ = case
    n, real = state[0], state[4]
    st, tr = pt.state_truth(state)
    pin = pt.pin_mask(n, mask)
    d = np.where(pin, np.inf, 0.0)
    v = _v(n).astype(real)
    mus = pt.shifts(case)
    assert any(pt.sees(case, mu) for mu in mus)
    for mu in mus:
        op, off = pt.shifted(tr, pin, mu), tr.shifted(d, mu * (1 + 1e-6), rec=True)
        ref, wrong = op.apply(v[None]), off.apply(v[None])
        gap = np.abs(wrong - ref).astype(np.float64)[0]
        b = op.bound_apply(v[None], real, ref)[0]
        bn = pt.bound_norm2(op, v)
        gn = abs(float(pt.norm2(off, v) - pt.norm2(op, v)))
        rs = float((gap[~pin] / b[~pin]).max())
        if pt.sees(case, mu):
            assert (gap > b).any(), (mu, rs)
            assert gn > bn, (mu, gn, bn)
        else:
            print("REAL32 mu %.3e, below MU32_SEES: solve gap / bound up to %.3g, ||x||^2 gap / bound %.3g"
                  % (mu, rs, gn / bn))
        if real == np.float64:
            bl = op.bound_logdet(op.sum_abs_log, op.cond_a)
            gl = abs(float(off.logdet - op.logdet))
        else:
            rt = pt.route_truth(state)
            rop, roff = pt.shifted(rt, pin, mu), rt.shifted(d, mu * (1 + 1e-6), rec=True)
            bl = 2 * rop.bound_logdet(rop.sum_abs_log, rop.cond_a)
            gl = abs(float(roff.logdet - rop.logdet))
        assert gl > bl, (mu, gl, bl)
