"""CPU: the float64 reference of tests/sage_ref.py against independent forms (F.normalize(F.linear) + F.batch_norm; autograd through
the whole composition from agg, W and b), the kink margins of the backward inputs, the float32 twin (oracle/flat_ref.TorchKernels)
on every case of tests/test_sage_fp64_gpu.py under the yardsticks of that file, and the bookkeeping that the case lists reach every
kernel instance and both sides of every dispatch condition.  e32, the twin's excess, is held to 0.25; an output that cannot meet that
in float32 carries its measured e32 in the table E32 below, and the GPU bound of that output in that case becomes max(1, 4 * e32).

    family     output         case                     e32 (measured)
    wide_fwd   mean           n31-K16-F1152-ldh1155    6.908
    wide_fwd   running_mean   n31-K16-F1152-ldh1155    6.909
    wide_fwd   running_mean   n32-K17-F1153-ldh1156    0.2503
    wide_fwd   mean           n63-K32-F1664-ldh1667    0.4838
    wide_fwd   running_mean   n63-K32-F1664-ldh1667    0.4856
    wide_fwd   mean           n97-K20-F1664-ldh1667    0.5432
    wide_fwd   running_mean   n97-K20-F1664-ldh1667    0.5445
    (everything else stays at or below 0.25, so its GPU bound is 1)

All entries are the pointwise column mean at few rows and many columns: with 31 to 97 rows of mean 1 and spread 1, one of more
than a thousand columns (times four activations, with and without normalize) has a mean that cancels to a part in a thousand, and
the float32 rounding of hn then shows in it.  The entries of E32 are the measured values rounded up by about 5 %."""
import pytest
import torch

import rowops_ref as R
import sage_ref as S
from oracle.flat_ref import TorchKernels

# (family, output, case name) -> e32 of the float32 twin; absent: e32 <= 0.25
E32 = {
    ('wide_fwd', 'mean', 'n31-K16-F1152-ldh1155'): 7.3,
    ('wide_fwd', 'running_mean', 'n31-K16-F1152-ldh1155'): 7.3,
    ('wide_fwd', 'running_mean', 'n32-K17-F1153-ldh1156'): 0.27,
    ('wide_fwd', 'mean', 'n63-K32-F1664-ldh1667'): 0.52,
    ('wide_fwd', 'running_mean', 'n63-K32-F1664-ldh1667'): 0.52,
    ('wide_fwd', 'mean', 'n97-K20-F1664-ldh1667'): 0.58,
    ('wide_fwd', 'running_mean', 'n97-K20-F1664-ldh1667'): 0.58,
}


def bound(family, name, case):
    """The bound of a GPU excess: 1, or 4 x the float32 twin's own excess where the table above records one."""
    return max(1.0, 4.0 * E32.get((family, name, case), 0.0))


TWIN = TorchKernels()


def bwd_name(case):
    return 'fin%d-F%d-n%d-%s' % case


# ---------------------------------------------------------------------------------------------- reference against independent forms
@pytest.mark.parametrize('K,F,n', [(7, 33, 37), (20, 20, 70), (32, 114, 37)])
@pytest.mark.parametrize('normalize', [True, False])
def test_reference_forward_is_linear_normalize_batch_norm(K, F, n, normalize):
    c = S.forward_inputs(K, F, n)
    count = float(n)
    for bias in (c.bias, None):
        ref = S.sage_forward(c.agg, c.W, bias, n, K, F, normalize, 2, count)
        h = torch.nn.functional.linear(c.agg.double(), c.W.double().t(), None if bias is None else bias.double())
        hn = torch.nn.functional.normalize(h, dim=1) if normalize else h
        rm, rv = torch.zeros(F, dtype=torch.float64), torch.ones(F, dtype=torch.float64)
        eps, mom = float(torch.tensor(R.BN_EPS, dtype=torch.float32)), float(torch.tensor(R.MOMENTUM, dtype=torch.float32))
        o = torch.nn.functional.elu(hn)
        y = torch.nn.functional.batch_norm(o, rm, rv, None, None, True, mom, eps)
        close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
        assert close(ref.hn, hn) and close(ref.running_mean, rm) and close(ref.running_var, rv)
        assert close((o - ref.mean) * ref.istd, y)
        assert close(ref.rinv, 1.0 / h.norm(dim=1) if normalize else torch.ones(n, dtype=torch.float64))
        assert bool((ref.hn_terms >= ref.hn.abs() * (1 - 1e-12)).all()) and ref.num_batches_tracked == 1


@pytest.mark.parametrize('fin,F,n', [(20, 20, 37), (7, 32, 37), (32, 5, 70)])
@pytest.mark.parametrize('act,normalize,mode', [(2, True, 2), (3, True, 1), (1, False, 0), (0, False, 2)])
def test_reference_backward_is_autograd_through_the_whole_layer(fin, F, n, act, normalize, mode):
    """y = BN(act(l2norm(agg W + b))) differentiated from agg, W and b by autograd, at h = agg W + b for the case's agg and W and a
    bias of 1 (sage_backward takes h as given: the case's own h is no product of its agg and W)."""
    c = S.backward_inputs(fin, F, n)
    agg, W = c.agg.double().requires_grad_(), c.W.double().requires_grad_()
    b = torch.ones(F, dtype=torch.float64, requires_grad=True)
    h = agg @ W + b
    ref = S.sage_backward(h.detach(), c.dy, c.agg, c.W, n, fin, F, act, normalize, mode, c.count, c.gamma, c.mean_run, c.istd_run)
    hn = torch.nn.functional.normalize(h, dim=1) if normalize else h
    o = R.activation(hn, act)
    if mode == 2:
        padded = torch.cat([o, torch.zeros(int(c.count) - n, F, dtype=torch.float64)])
        y = torch.nn.functional.batch_norm(padded, None, None, c.gamma.double(), ref.beta, True, 0.1,
                                           float(torch.tensor(R.BN_EPS, dtype=torch.float32)))[:n]
    elif mode == 1:
        y = (o - c.mean_run.double()) * c.istd_run.double() * c.gamma.double() + ref.beta
    else:
        y = o
    dagg, dW, db = torch.autograd.grad(y, [agg, W, b], c.dy.double())
    close = lambda a, b_: float((a - b_).abs().max()) <= 1e-11 * max(1.0, float(b_.abs().max()))
    assert close(ref.dagg, dagg) and close(ref.dW, dW) and close(ref.db, db)
    for v, t in ((ref.dagg, ref.dagg_terms), (ref.dW, ref.dW_terms), (ref.db, ref.db_terms)):
        assert bool((t >= v.abs() * (1 - 1e-9)).all())


# ---------------------------------------------------------------------------------------------- margins of the GPU inputs
def test_backward_inputs_keep_their_distance_from_the_kink():
    for fin, F, n, variant in S.NARROW_BWD_CASES:
        c = S.backward_inputs(fin, F, n, variant)
        assert R.margin_epilogue(c) >= R.MARGIN, (fin, F, n, variant)
        assert float(c.h.abs()[c.h != 0].min()) >= float(torch.tensor(0.01, dtype=torch.float32))
        if variant == 'b':
            assert n == R.N_BASE and float(c.h[3].abs().max()) == 0.0
        else:
            assert bool((c.h != 0).all())


# ---------------------------------------------------------------------------------------------- the float32 twin
def _launch(mis=()):
    return lambda run: run(S.Places('cpu', mis))


def _same_bits(a, b):
    return torch.equal(a, b)


def _hold(family, case, ex):
    print('SAGE twin %s %s: %s' % (family, case, ex.line()))
    bad = {name: e for name, e in ex.items() if not e <= E32.get((family, name, case), 0.25)}
    assert not bad, '%s %s: e32 above 0.25 or above its entry in E32: %r' % (family, case, bad)


@pytest.mark.parametrize('case', S.WIDE_CASES, ids=lambda c: c.name)
def test_twin_wide_forward(case):
    _hold('wide_fwd', case.name, S.check_forward_case(TWIN, case, _launch(case.mis)))


@pytest.mark.parametrize('case', S.NARROW_FWD_CASES, ids=lambda c: c.name)
def test_twin_narrow_forward(case):
    _hold('narrow_fwd', case.name, S.check_forward_case(TWIN, case, _launch()))


@pytest.mark.parametrize('case', S.ZERO_ROW_CASES, ids=lambda c: c.name)
def test_twin_zero_projection_row(case):
    _hold('zero_row', case.name, S.check_forward_case(TWIN, case, _launch(), zero_row=5, combos=[(True, False)]))


@pytest.mark.parametrize('case', S.NARROW_BWD_CASES, ids=bwd_name)
def test_twin_narrow_backward(case):
    _hold('narrow_bwd', bwd_name(case), S.check_backward_case(TWIN, case, _launch(), _same_bits))


# ---------------------------------------------------------------------------------------------- bookkeeping over the case lists
def test_case_list_visits_every_instance():
    """BOOKKEEPING: sage_ref.wide_dispatch / narrow_*_dispatch restate the host dispatch of cgc_sage_wide_fwd, sage_narrow_fwd_groups
    and sage_narrow_bwd_groups and have to follow it when it changes.  They are used here only: to assert that the case lists reach
    every reachable kernel instance, every grid-stride loop, and both sides of every condition of the cols route."""
    seen = set()
    for case in S.WIDE_CASES + S.NARROW_FWD_CASES:
        for nrm in (True, False):
            for stats in (True, False):
                d = S.case_dispatch(case, nrm, stats)
                for act in S.forward_acts(case):
                    if d.route == 'base':
                        seen.add(('base', d.KS, d.NTW))
                        seen.add(('base', 'small' if case.n < 64 else 'large'))
                    elif d.route == 'fwd8':
                        seen.add(('fwd8', d.KS, d.NTW, act))
                        seen.add(('fwd8', 'vector' if d.vector else 'scalar'))
                    elif d.route == 'cols':
                        seen.add(('cols', d.KS, act))
                        seen.add(('rinv', d.KK))
                        seen.add(('cols groups', d.groups, d.wgs_per_chunk))
                    else:
                        seen.add(('narrow_fwd', d.KS, act))
                seen.add((d.route, 'normalize', nrm))
                if d.strides:
                    seen.add((d.route, 'strides'))
    for fin, F, n, _ in S.NARROW_BWD_CASES:
        d = S.narrow_bwd_dispatch(n, fin, F)
        for act in S.backward_acts(n):
            seen.add(('narrow_bwd', d.FS, act))
        if d.strides:
            seen.add(('narrow_bwd', 'strides'))
    want = {('base', ks, ntw) for ks in (8, 10, 16) for ntw in (9, 13)} | {('base', 'small'), ('base', 'large')}
    want |= {('fwd8', ks, ntw, act) for ks in (8, 10) for ntw in (5, 7) for act in S.ACTS} | {('fwd8', 'vector'), ('fwd8', 'scalar')}
    want |= {('cols', ks, act) for ks in (9, 11) for act in S.ACTS} | {('rinv', kk) for kk in (16, 20, 32)}
    want |= {('cols groups', 1, 1), ('cols groups', 2, 1), ('cols groups', 5, 2)}
    want |= {('narrow_fwd', ks, act) for ks in (8, 10, 16) for act in S.ACTS}
    want |= {('narrow_bwd', fs, act) for fs in (8, 10, 16) for act in S.ACTS}
    want |= {(route, 'strides') for route in ('base', 'fwd8', 'cols', 'narrow_fwd', 'narrow_bwd')}
    want |= {(route, 'normalize', nrm) for route in ('base', 'fwd8', 'narrow_fwd') for nrm in (True, False)}
    assert not want - seen, 'instances no case reaches: %r' % sorted(want - seen, key=repr)
    # both sides of every condition of the cols route, on the same inputs
    for what, (inside, outside) in S.COLS_PAIRS.items():
        assert S.case_dispatch(inside, True).route == 'cols', what
        assert S.case_dispatch(outside, True).route != 'cols', what
        assert S.case_dispatch(inside, False).route != 'cols', what
    for case in S.WIDE_COLS:
        assert S.case_dispatch(case, True).route == 'cols' and S.case_dispatch(case, False).route != 'cols', case.name
    for case in S.WIDE_FWD8:
        assert S.case_dispatch(case, True).route == 'fwd8', case.name
    for case in S.WIDE_BASE:
        assert S.case_dispatch(case, True).route == 'base', case.name
    assert S.case_dispatch(S.WIDE_GRID[0], True).route == 'base' and S.case_dispatch(S.WIDE_GRID[1], False).route == 'fwd8'
    routes = [S.case_dispatch(c, True).route for c in S.ZERO_ROW_CASES]
    assert routes == ['base', 'fwd8', 'cols', 'narrow_fwd']
    # K in 21..32 never takes fwd8 (its [2 * 16][Fp] copy of W does not fit the LDS): the base kernel at every F below 12288 rows
    for K in range(21, 33):
        for F in range(33, 1665):
            for n in (64, 12287):
                assert S.wide_dispatch(n, K, F, F, K, True).route == 'base'
            assert S.wide_dispatch(12288, K, F, F, K, False).route == 'base'
            assert S.wide_dispatch(12288, K, F, F, K, True).route == ('cols' if K == 21 else 'base')
