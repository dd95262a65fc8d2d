"""Float64 reference of the SAGE projection kernels (csrc/sagewide.hip, csrc/sagenarrow.hip) for tests/test_sage_ref_cpu.py and
tests/test_sage_fp64_gpu.py, built from the parts of tests/rowops_ref.py: the forward is hn = l2norm(agg W + b) with the BatchNorm
statistics of act(hn) over `count` rows and one update of the running statistics from (0, 1); the backward is rowops_ref.epilogue()
on a given h followed by d agg = d h W^T, d W = agg^T d h, d b = colsum(d h).  Beside every output that is a cancelling sum the
reference returns ``*_terms``, the sum of the absolute values of its summands.

Beside the operators: the inputs and the case lists the GPU tests run (the CPU file pins the float32 twin on every one of them), the
call sequences (the same code drives the twin on the CPU and the HIP kernels), the judges, and ``wide_dispatch`` / ``narrow_*_dispatch``:
a restatement of the host dispatch that is BOOKKEEPING -- it only serves to assert that the case lists reach every kernel instance
and both sides of every dispatch condition, and has to follow csrc/ when the dispatch there changes."""
import ctypes
import math

import torch

import rowops_ref as R
from rowops_ref import Bag

ACTS = R.ACTS
BIG = 1000000                 # cases with more output elements run ReLU and ELU only
RINV_CLAMPED = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(1e-12, dtype=torch.float32))     # float32(1 / 1e-12f)


# ------------------------------------------------------------------------------------------------ operators in float64
def sage_forward(agg, W, bias, n, K, F, normalize, act, count, base=None):
    """-> Bag(h, hn, rinv, hn_terms, stats, stats_terms, mean, istd, running_mean, running_var, num_batches_tracked, zero_rows).
    hn_terms = rinv * (|agg| @ |W| + |b|): hn is a K-term sum that may cancel.  ``base``: an earlier result for the same operands
    and the same `normalize` (another activation), whose product and norms are reused."""
    if base is None:
        a, w = R._d(agg)[:n, :K], R._d(W)[:K, :F]
        h, ht = a @ w, a.abs() @ w.abs()
        if bias is not None:
            b = R._d(bias)
            h, ht = h + b, ht + b.abs()
        hn, rinv = R._l2norm(h, normalize)
        zero = torch.nonzero(torch.linalg.vector_norm(h, dim=1) < R.L2_EPS).flatten().tolist() if normalize else []
        base = Bag(h=h, hn=hn, rinv=rinv, hn_terms=rinv.unsqueeze(1) * ht, zero_rows=zero)
    o = R.activation(base.hn, act)
    stats = torch.stack([o.sum(0), (o * o).sum(0)])
    terms = torch.stack([o.abs().sum(0), (o * o).sum(0)])
    fin = R.bn_finalize(stats, count, R.BN_EPS, R.MOMENTUM, torch.zeros(F), torch.ones(F))
    return Bag(h=base.h, hn=base.hn, rinv=base.rinv, hn_terms=base.hn_terms, zero_rows=base.zero_rows, stats=stats, stats_terms=terms,
               mean=fin.mean, istd=fin.istd, running_mean=fin.running_mean, running_var=fin.running_var, num_batches_tracked=1)


def sage_backward(h, dy, agg, W, n, fin, F, act, normalize, mode, count, gamma, mean_run, istd_run):
    """rowops_ref.epilogue() on h at dy (its Bag, with hn, rinv, mean, istd, sums, dh, dh_terms, dhc, dhc_terms) plus
    dagg = dh W^T (dagg_terms = dh_terms |W|^T), dW = agg^T dh (dW_terms = |agg|^T dh_terms), db = dhc (db_terms = dhc_terms)."""
    e = R.epilogue(h, dy, n, F, act, normalize, mode, count, gamma, None, mean_run, istd_run)
    a, w = R._d(agg)[:n, :fin], R._d(W)
    e.dagg, e.dagg_terms = e.dh @ w.t(), e.dh_terms @ w.abs().t()
    e.dW, e.dW_terms = a.t() @ e.dh, a.abs().t() @ e.dh_terms
    e.db, e.db_terms = e.dhc, e.dhc_terms
    return e


# ------------------------------------------------------------------------------------------------ inputs
def forward_inputs(K, F, n, zero_row=None):
    """agg = N(0,1), W = N(0,1) / sqrt(K), bias = 1 + 0.3 N(0,1): the projection has a mean near 1 in every column, so that a column's
    mean does not cancel (with plain N(0,1) weights and bias it does, and float32 itself misses the pointwise yardstick).  The
    draws are nested: a case with fewer rows or a smaller K sees the leading rows / columns of the same draw, so the two sides of a
    dispatch condition on n or K get the same inputs."""
    agg = R._rnd(4000, n, 32)[:, :K].contiguous()
    W = (R._rnd(5000 + F, 32, F)[:K] / math.sqrt(K)).contiguous()
    if zero_row is not None:
        agg[zero_row] = 0.0
    return Bag(K=K, F=F, n=n, agg=agg, W=W, bias=1.0 + 0.3 * R._rnd(6000 + F, F), count=float(n + 17), rm0=torch.zeros(F),
               rv0=torch.ones(F), zero_row=zero_row)


def backward_inputs(fin, F, n, variant='a'):
    """h, dy, gamma, count and the constants of mode 1 as rowops_ref.epilogue_inputs (h = N(1,1), every entry at least 0.01 from the
    kink), agg = N(0,1) [n, fin], W = N(0,1) [fin, F].  variant 'a': no zero row; 'b': row 3 exactly zero."""
    c = R.epilogue_inputs(F, n)
    h = R._rnd(1000 + F, n, F) + 1.0
    h = torch.where(h < 0, -1.0, 1.0) * h.abs().clamp(min=0.01)
    c.zero_row = 3 if variant == 'b' else None
    if c.zero_row is not None:
        h[c.zero_row] = 0.0
    c.h, c.fin, c.variant = h, fin, variant
    c.agg, c.W = R._rnd(7000 + fin, n, fin), R._rnd(8000 + 33 * fin + F, fin, F)
    return c


# ------------------------------------------------------------------------------------------------ the host dispatch, restated
def _cdiv(a, b):
    return -(-a // b)


def _ks(K):
    return 8 if K <= 16 else 10 if K <= 20 else 16


def _cap(n):
    return min(_cdiv(max(n, 1), 4), 1024)


def gram_bytes(K):
    return 8 * (K * (K + 1) // 2 + K + 1)


def wide_dispatch(n, K, F, ldh, lda, normalize, stats=True, hn_off=0, rinv_off=0, w_off=0):
    """cgc_sage_wide_fwd's choice for a launch with n > 0 inside the envelope; *_off: the operand's offset from a 16-byte boundary
    in floats.  BOOKKEEPING: follows csrc/sagewide.hip."""
    ks, tiles, cap = _ks(K), _cdiv(n, 32), _cap(n)
    if (normalize and K <= 21 and n >= 12288 and n * ldh * 4 < 2 ** 31 and hn_off % 2 == 0 and rinv_off % 4 == 0
            and n * ldh * 4 >= gram_bytes(K) and ((n - 1) * lda + K) * 4 < 2 ** 31 and (ldh == F or F * 4 >= gram_bytes(K))):
        chunks = _cdiv(tiles, _cdiv(tiles, 256))
        if stats and chunks > cap:
            chunks = max(cap, 1)
        groups = _cdiv(_cdiv(F, 32), 3)
        return Bag(route='cols', KS=9 if K <= 17 else 11, KK={8: 16, 10: 20, 16: 32}[ks], strides=tiles > chunks, groups=groups,
                   wgs_per_chunk=_cdiv(groups, 4))
    ntw8 = 5 if F <= 1280 else 7
    lds8 = 4 * (2 * ks * 256 * ntw8 + 768)
    if ks <= 10 and F <= 1792 and lds8 <= 156 * 1024 and n >= 64 and n * ldh * 4 < 2 ** 31:
        wgs = min(tiles, 256)
        if stats and wgs > cap:
            wgs = max(cap, 1)
        return Bag(route='fwd8', KS=ks, NTW=ntw8, strides=tiles > wgs, vector=F % 4 == 0 and w_off % 4 == 0)
    wgs = min(tiles, 512)
    if stats and wgs > cap:
        wgs = max(cap, 1)
    return Bag(route='base', KS=ks, NTW=9 if F <= 1152 else 13, strides=tiles > wgs)


def narrow_fwd_dispatch(n, K, F, stats=True):
    """sage_narrow_fwd_groups.  BOOKKEEPING: follows csrc/sagenarrow.hip."""
    tiles = _cdiv(n, 32)
    grid = min(_cdiv(tiles, 4), 1024)
    if stats and grid > _cap(n):
        grid = max(_cap(n), 1)
    ks = (K + 1) // 2
    return Bag(route='narrow_fwd', KS=8 if ks <= 8 else 10 if ks <= 10 else 16, strides=tiles > 4 * grid)


def narrow_bwd_dispatch(n, fin, F):
    """sage_narrow_bwd_groups.  BOOKKEEPING: follows csrc/sagenarrow.hip."""
    tiles = _cdiv(n, 32)
    grid = min(_cdiv(tiles, 4), 1024)
    fs = (F + 1) // 2
    return Bag(route='narrow_bwd', FS=8 if fs <= 8 else 10 if fs <= 10 else 16, strides=tiles > 4 * grid)


# ------------------------------------------------------------------------------------------------ case lists
def wc(n, K, F, pad=3, mis=()):
    """A forward case: hn has the row stride F + pad (0: contiguous), the operands named in `mis` sit one float past a 16-byte
    boundary.  F <= 32 with pad = 0 is the narrow forward (cgc_sage_narrow_fwd)."""
    return Bag(n=n, K=K, F=F, ldh=F + pad, lda=K + 3, mis=tuple(mis),
               name='n%d-K%d-F%d-ldh%d%s' % (n, K, F, F + pad, ''.join('-' + m + 'mis' for m in mis)))


WIDE_BASE = [wc(1, 1, 33), wc(31, 16, 1152), wc(32, 17, 1153), wc(33, 20, 1664), wc(63, 21, 1152), wc(63, 32, 1664), wc(33, 16, 1153),
             wc(32, 20, 1152), wc(100, 21, 1153), wc(65, 32, 33)]
WIDE_FWD8 = [wc(64, 16, 1280), wc(65, 17, 1281), wc(97, 20, 1664), wc(64, 7, 257), wc(64, 7, 260), wc(64, 16, 1280, mis=('W',)),
             wc(66, 8, 1664), wc(70, 20, 1140)]
WIDE_COLS = [wc(12288, 7, 33, 0), wc(12301, 16, 96, 0), wc(12288, 17, 97, 0), wc(12301, 18, 385, 0), wc(12288, 20, 33, 0),
             wc(12301, 21, 97, 0), wc(12301, 20, 1140, 12)]
# both sides of every condition of the cols route on the same inputs: (the side that takes it, the side that does not)
COLS_PAIRS = {
    'n >= 12288': (wc(12288, 20, 96, 0), wc(12287, 20, 96, 0)),
    'K <= 21': (wc(12288, 21, 96, 0), wc(12288, 22, 96, 0)),
    'hn 8-byte aligned': (wc(12288, 20, 96, 0), wc(12288, 20, 96, 0, mis=('hn',))),
    'rinv 16-byte aligned': (wc(12288, 20, 96, 0), wc(12288, 20, 96, 0, mis=('rinv',))),
    'ldh == F or G fits row 0 (K=20: 1848 bytes against 1280)': (wc(12288, 20, 320, 0), wc(12288, 20, 320, 4)),
    'G fits row 0 (K=7: 288 bytes fit F=72, not F=71)': (wc(12288, 7, 72, 3), wc(12288, 7, 71, 3)),
}
WIDE_GRID = [wc(16417, 32, 64), wc(8225, 20, 64)]


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out


WIDE_CASES = _unique(WIDE_BASE + WIDE_FWD8 + WIDE_COLS + [c for pair in COLS_PAIRS.values() for c in pair] + WIDE_GRID)
NARROW_FWD_CASES = [wc(1, 1, 32, 0), wc(31, 2, 1, 0), wc(32, 15, 2, 0), wc(33, 16, 15, 0), wc(129, 17, 16, 0), wc(4100, 20, 17, 0),
                    wc(33, 21, 20, 0), wc(129, 31, 21, 0), wc(31, 32, 31, 0), wc(4100, 16, 32, 0), wc(131105, 20, 20, 0)]
# zero-projection row (bias None, one all-zero row of agg): once per route and on the narrow forward
ZERO_ROW_CASES = [wc(37, 20, 1140), wc(70, 20, 1140), wc(12301, 20, 96, 0), wc(37, 20, 20, 0)]
# (fin, F, n, variant)
NARROW_BWD_CASES = [(20, 20, 37, 'a'), (20, 20, 37, 'b'), (16, 16, 37, 'a'), (1, 32, 1, 'a'), (2, 15, 31, 'a'), (15, 16, 32, 'a'), (16, 17, 33, 'a'),
                    (17, 1, 129, 'a'), (21, 2, 129, 'a'), (31, 31, 33, 'a'), (32, 32, 37, 'a'), (32, 21, 4100, 'a'),
                    (20, 20, 131105, 'a')]


def case_dispatch(case, normalize, stats=True):
    if case.F <= 32 and case.ldh == case.F:
        return narrow_fwd_dispatch(case.n, case.K, case.F, stats)
    off = lambda name: 1 if name in case.mis else 0
    return wide_dispatch(case.n, case.K, case.F, case.ldh, case.lda, normalize, stats, off('hn'), off('rinv'), off('W'))


def forward_acts(case):
    return ACTS if case.n * case.F <= BIG else (1, 2)


def backward_acts(n):
    return ACTS if n == R.N_BASE else (1, 2)


# ------------------------------------------------------------------------------------------------ placement
class Places(object):
    """An aligned and a misaligned rowops_ref.Place; the operands named in `mis` go to the second."""

    def __init__(self, dev, mis=()):
        self.dev, self.a, self.m, self.mis = dev, R.Place(dev), R.Place(dev, 'misaligned'), frozenset(mis)

    def of(self, name):
        return self.m if name in self.mis else self.a

    def check(self):
        self.a.check(), self.m.check()


# ------------------------------------------------------------------------------------------------ call sequences
def run_forward(Kn, P, c, case, normalize, act, stats, with_bias):
    """One call of sage_wide_fwd on kernels Kn.  -> dict name -> tensor (plus 'ok')."""
    n, K, F = c.n, c.K, c.F
    agg = P.of('agg').inp(c.agg, case.lda)
    W = P.of('W').inp(c.W)
    bias = P.of('bias').inp(c.bias) if with_bias else None
    o = {'hn': P.of('hn').out(n, F, case.ldh), 'rinv': P.of('rinv').out(n)}
    rm = rv = nbt = mean = istd = None
    if stats:
        o['mean'], o['istd'] = mean, istd = P.a.out(F), P.a.out(F)
        o['rm'], o['rv'] = rm, rv = P.a.inp(c.rm0), P.a.inp(c.rv0)
        o['nbt'] = nbt = torch.zeros((), dtype=torch.int64, device=P.dev)
    ok = Kn.sage_wide_fwd(agg, case.lda, W, bias, n, K, F, normalize, act, o['hn'], o['rinv'], stats, c.count, R.BN_EPS, R.MOMENTUM,
                          rm, rv, nbt, mean, istd)
    assert ok, 'sage_wide_fwd refused a shape inside its envelope'
    return o


def judge_forward(c, ref, o, ex, with_bias, rows=True):
    """rows: judge hn and rinv (False: the caller saw the bits of an output already judged).  Without a bias the column means
    cancel (the projection is N(0,1) per entry), so `mean` and `running_mean` = 0.1 mean are judged as the sums they are:
    |a-b| <= 1e-4 * stats_terms / count + 1e-7."""
    if rows:
        ex.add('hn', R.excess_sum(o['hn'], ref.hn, ref.hn_terms))
        ex.add('rinv', R.excess_point(o['rinv'], ref.rinv))
    if 'mean' not in o:
        return
    if with_bias:
        ex.add('mean', R.excess_point(o['mean'], ref.mean))
        ex.add('running_mean', R.excess_point(o['rm'], ref.running_mean))
    else:
        t = ref.stats_terms[0] / c.count
        ex.add('mean_nobias', R.excess_sum(o['mean'], ref.mean, t))
        ex.add('running_mean_nobias', R.excess_sum(o['rm'], ref.running_mean, float(torch.tensor(R.MOMENTUM, dtype=torch.float32)) * t))
    ex.add('istd', R.excess_point(o['istd'], ref.istd))
    ex.add('running_var', R.excess_point(o['rv'], ref.running_var))
    assert int(o['nbt'].item()) == ref.num_batches_tracked == 1


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32) if a.is_contiguous() else a.contiguous().view(torch.int32),
                                              b.view(torch.int32) if b.is_contiguous() else b.contiguous().view(torch.int32))


def check_forward_case(Kn, case, launch, zero_row=None, combos=None):
    """Every (normalize, bias, activation, stats) combination of a forward case on kernels Kn: ``launch(run)`` calls run(Places) -> outputs (the GPU
    file launches twice and asserts containment and identical bits).  hn and rinv do not depend on the activation or on `stats`:
    they are judged in float64 once per (normalize, bias) and again whenever their bits differ from the ones judged.  -> Excess"""
    c = forward_inputs(case.K, case.F, case.n, zero_row)
    ex = R.Excess()
    for nrm, wb in (combos or [(a, b) for a in (True, False) for b in (True, False)]):
        ref, judged = None, None
        for act in forward_acts(case):
            ref = sage_forward(c.agg, c.W, c.bias if wb else None, c.n, c.K, c.F, nrm, act, c.count, base=ref)
            for stats in (True, False):
                o = launch(lambda P: run_forward(Kn, P, c, case, nrm, act, stats, wb))
                rows = judged is None or not (_same(o['hn'], judged['hn']) and _same(o['rinv'], judged['rinv']))
                judge_forward(c, ref, o, ex, wb, rows)
                if judged is None:
                    judged = o
                if zero_row is not None and nrm and not wb:
                    assert ref.zero_rows == [zero_row]
                    assert float(o['hn'][zero_row].abs().max()) == 0.0, 'the zero row of hn is not exactly zero'
                    assert float(o['rinv'][zero_row]) == RINV_CLAMPED, 'rinv of the zero row is not float32(1 / 1e-12f)'
    return ex


def backward_reference(c):
    """{(act, normalize, mode): sage_backward(...)} of a case."""
    return {(act, nrm, mode): sage_backward(c.h, c.dy, c.agg, c.W, c.n, c.fin, c.F, act, nrm, mode, c.count, c.gamma, c.mean_run,
                                            c.istd_run)
            for act in backward_acts(c.n) for nrm in (True, False) for mode in (2, 1, 0)}


def narrow_bwd_ldd(Kn, dy, ldy, hn, rinv, n, F, act, normalize, mode, mean, istd, gamma, sums, count, agg, lda, fin, W, dagg, ldd, dwdb):
    """sage_narrow_bwd with a free row stride of dagg (the wrapper always passes fin): the C entry point directly, its workspace sized
    by cgc_sage_narrow_ws_floats.  The float32 twin takes the stride from the view.  -> False where the entry point refuses."""
    if not hasattr(Kn, 'lib'):
        return Kn.sage_narrow_bwd(dy, ldy, hn, rinv, n, F, act, normalize, mode, mean, istd, gamma, sums, count, agg, lda, fin, W, dagg,
                                  dwdb)
    Kn._dev(dy, hn, rinv, mean, istd, gamma, sums, agg, W, dagg, dwdb)
    ws = torch.empty(int(Kn.lib.cgc_sage_narrow_ws_floats(n, fin, F)), dtype=torch.float32, device=dwdb.device)
    p = lambda t: None if t is None else t.data_ptr()
    rc = Kn.lib.cgc_sage_narrow_bwd(p(dy), ldy, p(hn), p(rinv), n, F, act, int(normalize), mode, p(mean), p(istd), p(gamma), p(sums),
                                    ctypes.c_double(count), p(agg), lda, fin, p(W), p(dagg), ldd, p(dwdb), p(ws), Kn._stream())
    if rc == -1:
        return False
    assert rc == 0, 'cgc_sage_narrow_bwd failed with code %d' % rc
    return True


def run_backward(Kn, P, c, refs, act, nrm, mode):
    """sage_narrow_bwd three times: dagg with ldd = fin + 3, with ldd = fin, and without dagg.  The kernel consumes saved forward
    outputs and the reduced sums: it gets the float32 roundings of the float64 reference's own."""
    n, F, fin = c.n, c.F, c.fin
    r = refs[(act, nrm, mode)]
    P = P.a
    hn32, rinv32 = P.inp(R.f32(r.hn)), P.inp(R.f32(r.rinv))
    dy, agg, W = P.inp(c.dy, F + 8), P.inp(c.agg, fin + 5), P.inp(c.W)
    mean32, istd32, gamma = (P.inp(R.f32(r.mean)), P.inp(R.f32(r.istd)), P.inp(c.gamma)) if mode else (None, None, None)
    sums32 = P.inp(R.f32(r.sums)) if mode == 2 else None
    o = {}
    for tag, ldd in (('wide', fin + 3), ('tight', fin), ('none', None)):
        dagg = None if ldd is None else P.out(n, fin, ldd)
        o['dwdb_' + tag] = P.out(fin * F + F)
        if ldd is not None:
            o['dagg_' + tag] = dagg
        args = (dy, F + 8, hn32, rinv32, n, F, act, nrm, mode, mean32, istd32, gamma, sums32, c.count, agg, fin + 5, fin, W, dagg)
        if ldd == fin + 3:
            ok = narrow_bwd_ldd(Kn, *(args + (ldd, o['dwdb_' + tag])))
        else:
            ok = Kn.sage_narrow_bwd(*(args + (o['dwdb_' + tag],)))
        assert ok, 'sage_narrow_bwd refused a shape inside its envelope'
    return o


def judge_backward(c, r, o, ex):
    """variant 'a': dagg, dW and db under the sum yardstick -- this is what pins dW and db.  variant 'b' (row 3 of h zero): under
    `normalize` dagg is judged row by row with the clamped row on its own terms (under its own name); the terms of dW and db then
    contain that row's 1e12 summand, so their check in this variant is loose by construction."""
    n, F, fin = c.n, c.F, c.fin
    keep = torch.ones(n, dtype=torch.bool)
    for row in r.zero_rows:
        keep[row] = False
    for tag in ('wide', 'tight'):
        dagg = o['dagg_' + tag].detach().cpu()
        ex.add('dagg', R.excess_sum(dagg[keep], r.dagg[keep], r.dagg_terms[keep]))
        if not bool(keep.all()):
            ex.add('dagg_zero_row', R.excess_sum(dagg[~keep], r.dagg[~keep], r.dagg_terms[~keep]))
    loose = '' if bool(keep.all()) else '_with_zero_row'
    dwdb = o['dwdb_wide'].detach().cpu()
    ex.add('dW' + loose, R.excess_sum(dwdb[:fin * F].view(fin, F), r.dW, r.dW_terms))
    ex.add('db' + loose, R.excess_sum(dwdb[fin * F:], r.db, r.db_terms))


def check_backward_case(Kn, case, launch, same_bits):
    fin, F, n, variant = case
    c = backward_inputs(fin, F, n, variant)
    refs = R.cached('sage_bwd_%s_%d' % (variant, fin), F, n, lambda: backward_reference(c))
    ex = R.Excess()
    for (act, nrm, mode), r in sorted(refs.items()):
        o = launch(lambda P: run_backward(Kn, P, c, refs, act, nrm, mode))
        assert same_bits(o['dagg_wide'], o['dagg_tight']), 'dagg depends on its row stride'
        assert same_bits(o['dwdb_wide'], o['dwdb_tight']) and same_bits(o['dwdb_wide'], o['dwdb_none']), 'dwdb depends on dagg'
        judge_backward(c, r, o, ex)
    return ex
