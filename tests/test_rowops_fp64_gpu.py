"""GPU: every row kernel of csrc/rowops.hip against the float64 reference of tests/rowops_ref.py, element by element, at one width
per (VEC, MAXJ, lanes-per-row) class of col_cfg() and on every route (register-resident, three-pass streaming, forced scalar lanes).

Yardsticks (tests/rowops_ref.py): pointwise outputs (hn, rinv, y, mean, istd, running statistics, softmax, An, At, invd, the
re-normalised adjacency) purely relative, |a-b| <= 1e-5 |b|, and exactly zero where the reference is; cancelling sums (column sums,
sums, dh, dhc, softmax backward and its column sums, dA) by |a-b| <= 1e-4 * terms + 1e-7 with terms the sum of |summands|.  An
excess is the largest ratio of an error to its allowance; each is bounded by max(1, 4 * e32) with e32 from the table of
tests/test_rowops_ref_cpu.py (the float32 twin stays below 0.25 everywhere, so every bound is 1) and printed.

Per case also: nothing is written outside an output (canary-filled wider buffers), a second launch repeats every bit, the in-place
softmax and the variants without fused column sums give the bits of their siblings, and beyond 2048 columns the entry points either
compute on the streaming route or refuse without touching their outputs."""
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
import rowops_ref as R
from test_rowops_ref_cpu import ADJ_WIDTHS, EPILOGUE_CASES, bound

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

ROW_CASES = ([(w, n, 'aligned') for w, n in R.row_cases()]
             + [(w, R.N_BASE, v) for w in R.FORCED_WIDTHS for v in ('misaligned', 'ld1')])
SOFTMAX_CASES = ROW_CASES + [(w, R.N_BASE, 'aligned') for w in R.BEYOND_WIDTHS]
ADJ_CASES = [(w, 'aligned') for w in ADJ_WIDTHS] + [(w, 'misaligned') for w in R.FORCED_WIDTHS]


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    as_int = torch.int64 if a.element_size() == 8 else torch.int32
    return a.shape == b.shape and torch.equal(a.view(as_int), b.view(as_int))


def twice(run):
    """run(Place) -> outputs, launched twice on fresh buffers: containment both times, identical bits."""
    first, second = R.Place(DEV, run.variant), R.Place(DEV, run.variant)
    o1, o2 = run(first), run(second)
    torch.cuda.synchronize()
    first.check(), second.check()
    for key in o1:
        assert same_bits(o1[key], o2[key]), 'second launch differs: ' + key
    return o1


def hold(family, what, width, ex):
    print('ROWOPS %s %s: %s' % (family, what, ex.line()))
    bad = {k: (e, bound(family, k, width)) for k, e in ex.items() if not e <= bound(family, k, width)}
    assert not bad, '%s %s: excess above its bound: %r' % (family, what, bad)


@pytest.mark.parametrize('F,n,variant', ROW_CASES)
def test_conv_epilogue_and_batchnorm(F, n, variant):
    """l2norm_act_stats, bn_finalize, l2norm_act_bn, bn_act_apply, bn_bwd_reduce, bn_act_l2_bwd (modes 0, 1, 2; with and without
    normalize; with and without the fused column sums) and colsum."""
    k = hip()
    c = R.epilogue_inputs(F, n)
    refs = R.cached('epilogue', F, n, lambda: R.epilogue_reference(c))
    ex = R.Excess()
    for act in R.case_acts(n):
        for nrm in (True, False):
            run = lambda P: R.run_epilogue(k, P, c, refs, act, nrm)
            run.variant = variant
            o = twice(run)
            for mode in ('2', '1', '0'):
                assert same_bits(o['dh' + mode], o['dhn' + mode]), 'dh depends on the fused column sums'
            R.judge_epilogue(c, refs, act, nrm, o, ex)
    hold('epilogue', 'F=%d n=%d %s' % (F, n, variant), F, ex)


@pytest.mark.parametrize('C,n,variant', SOFTMAX_CASES)
def test_softmax(C, n, variant):
    k = hip()
    c = R.softmax_inputs(C, n)
    ref = R.cached('softmax', C, n, lambda: R.softmax_bwd(c.x, c.dS, n, C))
    beyond = C > 2048
    run = lambda P: R.run_softmax(k, P, c, ref, beyond=beyond)
    run.variant = variant
    o = twice(run)
    assert same_bits(o['S'], o['S_inplace']), 'in-place softmax differs from out-of-place'
    if not beyond:
        assert same_bits(o['dx'], o['dxn']), 'dx depends on the fused column sums'
    ex = R.Excess()
    R.judge_softmax(ref, o, ex)
    hold('softmax', 'C=%d n=%d %s' % (C, n, variant), C, ex)


@pytest.mark.parametrize('C,variant', ADJ_CASES)
def test_dense_adjacency(C, variant):
    """dense_rownorm, dense_renorm and adj_prep (with and without the re-normalisation, with and without the second gradient stream),
    forward and backward, on R = B * C rows."""
    k = hip()
    c = R.adjacency_inputs(C)
    ref = R.cached('adjacency', C, 0, lambda: R.adjacency_reference(c))
    run = lambda P: R.run_adjacency(k, P, c, ref)
    run.variant = variant
    o = twice(run)
    ex = R.Excess()
    R.judge_adjacency(ref, o, ex)
    hold('adjacency', 'C=%d B=%d %s' % (C, c.B, variant), C, ex)


@pytest.mark.parametrize('F', R.BEYOND_WIDTHS)
def test_entries_refuse_rows_wider_than_2048(F):
    """The column-reduction entry points have no instance for more than 2048 columns: they raise and leave their outputs alone."""
    k = hip()
    n = R.N_BASE
    P = R.Place(DEV)
    x, v = P.inp(torch.ones(n, F)), P.inp(torch.ones(F))
    row, sums = P.inp(torch.ones(n)), P.inp(torch.ones(2, F))
    calls = [
        lambda: k.l2norm_act_stats(x, n, F, True, 1, P.out(n, F), P.out(n), P.out(2, F, dtype=torch.float64)),
        lambda: k.l2norm_act_bn(x, n, F, True, 1, P.out(n, F), P.out(n), float(n), 1e-5, 0.1, P.out(F), P.out(F), None, P.out(F),
                                P.out(F)),
        lambda: k.bn_act_apply(x, n, F, 1, v, v, v, v, P.out(n, F), F),
        lambda: k.bn_bwd_reduce(x, F, x, n, F, 1, v, v, P.out(2, F)),
        lambda: k.bn_act_l2_bwd(x, F, x, row, n, F, 1, True, 2, v, v, v, sums, float(n), P.out(n, F), P.out(F)),
        lambda: k.bn_act_l2_bwd(x, F, x, row, n, F, 1, True, 2, v, v, v, sums, float(n), P.out(n, F)),
        lambda: k.colsum(x, F, n, F, P.out(F)),
        lambda: k.softmax_bwd(x, x, n, F, P.out(n, F), P.out(F)),
        lambda: k.softmax_bwd(x, x, n, F, P.out(n, F)),
    ]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert len(P.watch) >= 18
    for buf, _ in P.watch:
        got = buf.cpu()
        assert torch.equal(got, torch.full_like(got, R.CANARY)), 'a refusing entry point wrote to an output'


def test_case_lists_match_the_cpu_file():
    """Every (width, n) run here has its margins asserted and its float32 twin measured in tests/test_rowops_ref_cpu.py."""
    assert {(w, n) for w, n, _ in ROW_CASES} == set(EPILOGUE_CASES)
