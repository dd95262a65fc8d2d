"""GPU: the SAGE projection kernels of csrc/sagewide.hip (k_sage_wide_fwd, k_sage_wide_fwd8, k_sage_gram + k_sage_rinv +
k_sage_wide_cols) and csrc/sagenarrow.hip (k_sage_narrow_fwd, k_sage_narrow_bwd) against the float64 reference of tests/sage_ref.py,
element by element, on every route and kernel instance the host dispatch can select and on both sides of every condition of the
cols route (tests/test_sage_ref_cpu.py asserts that the case lists reach them).

Yardsticks (tests/rowops_ref.py): rinv, mean, istd and the running statistics purely relative, |a-b| <= 1e-5 |b|, and exactly zero
where the reference is; hn, dagg, dW, db (and the mean of a projection without bias, which cancels) as sums, |a-b| <= 1e-4 * terms +
1e-7 with terms the sum of |summands|; num_batches_tracked exact.  An excess is the largest ratio of an error to its allowance; each is
bounded by max(1, 4 * e32) with e32 from the table E32 of tests/test_sage_ref_cpu.py, and printed.

Per case: every combination of normalize, bias / no bias, statistics on / off and the activations; every output sits in a
canary-filled buffer with spare rows (and a row stride above its width where the route allows one); each launch runs twice on fresh
buffers, with containment asserted both times and identical bits.

Which case reaches what (case names are n-K-F-ldh; asserted by test_case_list_visits_every_instance of the CPU file):

    k_sage_wide_fwd<KS,NTW>      <8,9> n31-K16-F1152   <8,13> n33-K16-F1153   <10,9> n32-K20-F1152   <10,13> n32-K17-F1153, n33-K20-F1664
                                 <16,9> n63-K21-F1152  <16,13> n63-K32-F1664, n100-K21-F1153 (n >= 64)   grid-stride: n16417-K32-F64
    k_sage_wide_fwd8<KS,NTW,*>   <8,5> n64-K16-F1280 (also with W misaligned: scalar staging), n64-K7-F257 (scalar), n64-K7-F260 (vector)
                                 <8,7> n66-K8-F1664   <10,5> n70-K20-F1140   <10,7> n65-K17-F1281, n97-K20-F1664   grid-stride: n8225-K20-F64
    k_sage_wide_cols<KS,*>       <9> n12288-K7-F33 (1 group, 3 idle waves), n12301-K16-F96, n12288-K17-F97 (bias row in the last slot; 2 groups)
                                 <11> n12301-K18-F385 (2 workgroups per chunk), n12288-K20-F33, n12301-K21-F97, n12301-K20-F1140-ldh1152
    k_sage_rinv<KK>              <16> K = 7, 16   <20> K = 17, 18, 20   <32> K = 21
    k_sage_narrow_fwd<KS,*>      <8> K = 1, 2, 15, 16   <10> K = 17, 20   <16> K = 21, 31, 32   second tile per wave: n131105-K20-F20
    k_sage_narrow_bwd<FS,*>      <8> F = 1, 2, 15, 16   <10> F = 17, 20   <16> F = 21, 31, 32   second tile per wave: fin20-F20-n131105
    all four activations: every case up to 1e6 output elements (each instance above has one); ReLU and ELU beyond

    condition of the cols route    takes it                 does not (same inputs)
    n >= 12288                     n12288-K20-F96           n12287-K20-F96 (fwd8)
    K <= 21                        n12288-K21-F96           n12288-K22-F96 (base)
    normalize                      every cols case          the same case with normalize off
    hn 8-byte aligned              n12288-K20-F96           the same with hn one float off
    rinv 16-byte aligned           n12288-K20-F96           the same with rinv one float off
    ldh == F or G fits row 0       n12288-K20-F320-ldh320   n12288-K20-F320-ldh324 (1848 bytes against 1280)
    G fits row 0 (ldh > F)         n12288-K7-F72-ldh75      n12288-K7-F71-ldh74 (288 bytes against 284)

Measured on an MI355X: hn <= 0.004, rinv <= 0.018 (0.006 on the cols route, whose norms come from the float64 quadratic form), istd <=
0.025, running_var <= 0.011, dagg, dW, db <= 0.004 of their allowances; the pointwise mean stays below 0.4 except in the two cases
that E32 bounds above 1: n31-K16-F1152 (12.6 against 29.2) and n97-K20-F1664 (2.05 against 2.32)."""
import ctypes

import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
import rowops_ref as R
import sage_ref as S
from test_sage_ref_cpu import bound, bwd_name

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    as_int = torch.int64 if a.element_size() == 8 else torch.int32
    return a.shape == b.shape and torch.equal(a.view(as_int), b.view(as_int))


def twice(mis=()):
    """launch(run): run(Places) -> outputs, twice on fresh buffers: containment both times, identical bits."""
    def launch(run):
        first, second = S.Places(DEV, mis), S.Places(DEV, mis)
        o1, o2 = run(first), run(second)
        torch.cuda.synchronize()
        first.check(), second.check()
        for key in o1:
            assert same_bits(o1[key], o2[key]), 'second launch differs: ' + key
        return o1
    return launch


def hold(family, case, ex):
    print('SAGE %s %s: %s' % (family, case, ex.line()))
    bad = {k: (e, bound(family, k, case)) for k, e in ex.items() if not e <= bound(family, k, case)}
    assert not bad, '%s %s: excess above its bound: %r' % (family, case, bad)


@pytest.mark.parametrize('case', S.WIDE_CASES, ids=lambda c: c.name)
def test_wide_forward(case):
    """cgc_sage_wide_fwd on the base, fwd8 and cols routes (the route of a case: sage_ref.case_dispatch)."""
    hold('wide_fwd', case.name, S.check_forward_case(hip(), case, twice(case.mis)))


@pytest.mark.parametrize('case', S.NARROW_FWD_CASES, ids=lambda c: c.name)
def test_narrow_forward(case):
    """cgc_sage_narrow_fwd, reached through sage_wide_fwd with F <= 32 and a contiguous hn."""
    hold('narrow_fwd', case.name, S.check_forward_case(hip(), case, twice()))


@pytest.mark.parametrize('case', S.ZERO_ROW_CASES, ids=lambda c: c.name)
def test_zero_projection_row(case):
    """bias None and an all-zero row of agg, once per route: hn exactly 0 in that row and rinv == float32(1 / 1e-12f) -- on the cols
    route that value comes out of the quadratic form (sage_ref.check_forward_case asserts both)."""
    hold('zero_row', case.name, S.check_forward_case(hip(), case, twice(), zero_row=5, combos=[(True, False)]))


@pytest.mark.parametrize('case', S.NARROW_BWD_CASES, ids=bwd_name)
def test_narrow_backward(case):
    """cgc_sage_narrow_bwd: modes 0, 1, 2, with and without normalize; dagg with ldd = fin + 3 (the C entry point directly), with
    ldd = fin and absent -- dagg and dwdb carry the same bits whichever way, the columns between fin and ldd keep the canary."""
    hold('narrow_bwd', bwd_name(case), S.check_backward_case(hip(), case, twice(), same_bits))


def _untouched(P):
    for buf, _ in P.watch:
        got = buf.cpu()
        assert torch.equal(got, torch.full_like(got, R.CANARY)), 'a refusing entry point wrote to an output'


def test_wide_forward_refuses_outside_its_envelope():
    """K = 33, F = 1665 and ldh < F: False (or an error) and every output still at its canary."""
    k = hip()
    n = 37
    P = R.Place(DEV)
    for K, F, short in ((33, 64, False), (20, 1665, False), (20, 64, True)):
        agg, W, bias = P.inp(torch.ones(n, K)), P.inp(torch.ones(K, F)), P.inp(torch.ones(F))
        full = P.out(n, F)
        hn = full.as_strided((n, F), (F - 1, 1), full.storage_offset()) if short else full
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        try:
            ok = k.sage_wide_fwd(agg, K, W, bias, n, K, F, True, 1, hn, P.out(n), True, float(n), R.BN_EPS, R.MOMENTUM, P.out(F), P.out(F),
                                 nbt, P.out(F), P.out(F))
        except RuntimeError:
            ok = False
        assert ok is False, (K, F, short)
        assert int(nbt.item()) == 0
    torch.cuda.synchronize()
    assert len(P.watch) == 18
    _untouched(P)


def _raw_forward(k, narrow, agg, lda, W, bias, n, K, F, hn, ldh, rinv, count, rm, rv, nbt, mean, istd):
    """The C entry points themselves (the wrapper picks one from the stride of hn, which an empty view does not carry)."""
    p = lambda t: None if t is None else t.data_ptr()
    ws = torch.empty(int(k.lib.cgc_stats_ws_floats(n, F)), dtype=torch.float32, device=DEV)
    tail = (1, p(ws), ctypes.c_double(count), ctypes.c_float(R.BN_EPS), ctypes.c_float(R.MOMENTUM), p(rm), p(rv), p(nbt), p(mean), p(istd),
            k._stream())
    if narrow:
        return k.lib.cgc_sage_narrow_fwd(p(agg), lda, p(W), p(bias), n, K, F, 1, 1, p(hn), p(rinv), *tail)
    return k.lib.cgc_sage_wide_fwd(p(agg), lda, p(W), p(bias), n, K, F, 1, 1, p(hn), ldh, p(rinv), *tail)


@pytest.mark.parametrize('narrow,F', [(False, 64), (True, 20)])
def test_forward_with_nothing_to_do(narrow, F):
    """F = 0: success, nothing written.  n = 0: success, hn and rinv untouched; with statistics on, k_stats_finalize folds zero slots:
    mean = 0, istd = 1 / sqrt(eps) and one running-statistics update towards (0, 0) -- the float64 reference of an empty batch among
    `count` rows -- and num_batches_tracked = 1."""
    k = hip()
    K, count = 20, 17.0
    c = S.forward_inputs(K, F, 0)
    P = R.Place(DEV)
    agg37, W, bias = P.inp(torch.ones(37, K)), P.inp(c.W), P.inp(c.bias)
    hn, rinv, mean, istd, rm, rv = P.out(37, F, F + (0 if narrow else 3)), P.out(37), P.out(F), P.out(F), P.out(F), P.out(F)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    assert _raw_forward(k, narrow, agg37, K, W, bias, 37, K, 0, hn, hn.stride(0), rinv, count, rm, rv, nbt, mean, istd) == 0
    torch.cuda.synchronize()
    _untouched(P)
    assert int(nbt.item()) == 0
    rm, rv = P.inp(c.rm0), P.inp(c.rv0)
    assert _raw_forward(k, narrow, agg37, K, W, bias, 0, K, F, hn, hn.stride(0), rinv, count, rm, rv, nbt, mean, istd) == 0
    torch.cuda.synchronize()
    P.check()
    for t in (hn, rinv):
        assert float(t.min()) == R.CANARY and float(t.max()) == R.CANARY
    ref = S.sage_forward(c.agg, c.W, c.bias, 0, K, F, True, 1, count)
    assert float(ref.mean.abs().max()) == 0.0 and float(ref.running_mean.abs().max()) == 0.0
    assert float(mean.abs().max()) == 0.0 and float(rm.abs().max()) == 0.0
    assert torch.equal(istd.cpu(), R.f32(ref.istd))
    assert R.excess_point(rv, ref.running_var) <= 1.0
    assert int(nbt.item()) == 1


def test_narrow_backward_refusals_and_empty_batch():
    """fin = 33, F = 33 and ldd < fin with dagg given: refused, outputs untouched.  n = 0: dwdb is zeroed, nothing else written."""
    k = hip()
    n = 37
    P = R.Place(DEV)
    t = lambda *shape: P.inp(torch.ones(*shape))
    for fin, F, ldd in ((33, 20, 33), (20, 33, 20), (20, 20, 19)):
        dagg, dwdb = P.out(n, fin), P.out(fin * F + F)
        ok = S.narrow_bwd_ldd(k, t(n, F), F, t(n, F), t(n), n, F, 1, True, 2, t(F), t(F), t(F), t(2, F), float(n), t(n, fin), fin, fin,
                              t(fin, F), dagg, ldd, dwdb)
        assert ok is False, (fin, F, ldd)
    torch.cuda.synchronize()
    _untouched(P)
    fin = F = 20
    Q = R.Place(DEV)
    dagg, dwdb = Q.out(0, fin, fin + 3), Q.out(fin * F + F)
    ok = S.narrow_bwd_ldd(k, t(0, F), F, t(0, F), t(0), 0, F, 1, True, 2, t(F), t(F), t(F), t(2, F), 17.0, t(0, fin), fin, fin, t(fin, F),
                          dagg, fin + 3, dwdb)
    torch.cuda.synchronize()
    assert ok is True
    Q.check()
    assert float(dwdb.abs().max()) == 0.0

