"""GPU: the DiffPool regulariser kernels (csrc/diffpool_reg.hip) against the float64 reference of tests/reg_ref.py, kernel by kernel
and, where the output is per element, element by element.  The yardsticks are derived there (the device logf measured, see its table);
tests/test_reg_ref_cpu.py asserts that the cases reach both k_reg_entropy instances, a second pass of every grid-stride and lane
loop, the vector and scalar paths of k_reg_sumsq with and without a tail, the CSR route and T <= 0, that the float32 twins pass the
judges and that every mutant is rejected.

Every call goes straight to the library; outputs sit in canary-surrounded buffers; each case runs twice on fresh buffers and must give
identical bits.  An excess is an error over its allowance; the largest per kernel is printed.

Measured on an MI355X, the largest excess per kernel over all cases: k_reg_entropy<4> 0.093, k_reg_entropy<1> 0.067, k_reg_sumsq 0.674,
k_reg_trace 0.871, k_reg_finalize 0.871 (the last three are the float32 rounding of link and keep: the float32 twin gives the same
figures), k_reg_entropy_bwd<4> and <1> 0.377 each, k_reg_adj_bwd 0.918 with accumulate and bit for bit without, bwd_prep bit for bit.
The device's g(s) = -logf(s + eps) - s / (s + eps) is within 3.668 units of u (|log| + |ratio|) over the sweep (the worst at
s = 1.87e-21, where the logarithm is -34.5: about two units in its last place); 8 units are granted."""
import numpy as np
import pytest

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
import reg_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def twice(run, variant='aligned'):
    """run(Place) -> tuple of numpy arrays / scalars, twice on fresh buffers: containment both times, identical bits."""
    first, second = R.Place(DEV, variant), R.Place(DEV, variant)
    o1, o2 = run(first), run(second)
    first.check(), second.check()
    for a, b in zip(o1, o2):
        assert np.array_equal(bits(a), bits(b)), 'the second launch differs from the first'
    return o1


@pytest.mark.parametrize('name', list(R.forward_cases()))
def test_forward(name):
    c = R.forward_cases()[name]
    link, ent, keep = twice(lambda P: R.run_forward(hip(), P, c))
    ex = R.Excess()
    R.judge_forward(c, R.forward(c), link, ent, keep, ex)
    print('REG fwd %s: %s' % (name, ex.line()))
    assert all(e <= 1.0 for e in ex.values()), ex


def test_entropy_gradient_sweep():
    """The measurement behind LOGF_GRANTED, asserted: g(s) = -logf(s + eps) - s / (s + eps) over the sweep, through both instances."""
    S = R.sweep()
    g, unit = R.ent_grad64(S)
    worst = {}
    for rows, variant in ((R.Rows(S.shape[0], 64, 64, 0), 'aligned'), (R.Rows(S.shape[0], 64, 64, 1), 'misaligned')):
        got, = twice(lambda P: (R.run_entropy_bwd(hip(), P, S, rows, 1.0, np.zeros_like(S), 64),), variant)
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - g) / (R.U * unit)
        at = np.unravel_index(np.argmax(err), err.shape)
        worst[variant] = float(err.max())
        print('REG logf sweep (%s): %.3f units at s = %r' % (variant, err.max(), float(S[at])))
    assert max(worst.values()) <= R.LOGF_GRANTED


@pytest.mark.parametrize('B,C', R.PREP_BC)
def test_bwd_prep(B, C):
    G = R._rnd([B, C], B * C * C)
    d_ao = R._rnd([C, B], B * C * C)
    for d_reg, keep, given in (((0.7, -1.3), 2.5, True), ((0.7, -1.3), 2.5, False), ((0.7, 0.9), 0.0, True)):
        da = d_ao if given else None
        coef, dao, Gs = twice(lambda P: R.run_bwd_prep(hip(), P, d_reg, keep, 96.0, 12.0, da, G, B, C))
        wcoef, wdao, wGs = R.bwd_prep(d_reg, keep, 96.0, 12.0, da, G, B, C)
        assert np.array_equal(bits(coef), bits(wcoef)), (coef, wcoef)
        assert np.array_equal(bits(dao), bits(wdao)) and np.array_equal(bits(Gs), bits(wGs))
        if keep == 0.0:
            assert coef[0] == 0 and not Gs.any() and np.array_equal(bits(dao), bits(d_ao.reshape(B, C, C)))


@pytest.mark.parametrize('rows', R.ROW_CASES_BWD, ids=lambda r: 'n%d-C%d-ld%d-off%d' % r)
def test_entropy_bwd(rows):
    S = R.rows_matrix(rows.n, rows.C)
    ds0 = R._rnd([rows.n, rows.C, 1], rows.n, rows.C)
    ex = R.Excess()
    for ldd, variant in ((rows.ld, 'aligned'), (rows.ld + 4, 'aligned'), (rows.ld, 'misaligned')):
        route = R.route_rows(rows.n, rows.C, rows.ld, rows.off == 0, cap=R.source_constants().ent_bwd_cap)
        vec = route.vec if ldd % 4 == 0 and variant == 'aligned' else 1
        got, = twice(lambda P: (R.run_entropy_bwd(hip(), P, S, rows, -0.37, ds0, ldd),), variant)
        ex.add('k_reg_entropy_bwd<%d>' % vec, R.judge_entropy_bwd(S, -0.37, ds0, got))
    print('REG entropy_bwd n%d-C%d-ld%d-off%d: %s' % (rows + (ex.line(),)))
    assert all(e <= 1.0 for e in ex.values()), ex


@pytest.mark.parametrize('m', R.ADJ_M)
def test_adj_bwd(m):
    A, gA0 = R._rnd([m, 1], m), R._rnd([m, 2], m)
    ex = R.Excess()
    for accumulate in (0, 1):
        got, = twice(lambda P: (R.run_adj_bwd(hip(), P, A, 0.3, gA0, accumulate),))
        ex.add('k_reg_adj_bwd/acc%d' % accumulate, R.judge_adj_bwd(A, 0.3, gA0, accumulate, got))
    print('REG adj_bwd m=%d: %s' % (m, ex.line()))
    assert all(e <= 1.0 for e in ex.values()), ex
