"""GPU: the exact fp32 GEMM of csrc/gemm.hip and csrc/gemm_common.hpp (k_gemm_f32<FAST>, k_gemm_f32<!FAST>, k_gemm_f32_shortk on six tile
shapes and three layouts, k_gemm_fixup, the TileMap modes, the ragged modes, the extra K segments) and the reduce kernels
(k_reduce_batch_sum, k_reduce_many_parts) against the float64 reference of tests/gemm_ref.py, element by element, on every kernel
instance and route (tests/test_gemm_ref_cpu.py asserts that the case list reaches them, and that the check notices a dropped or doubled
k, a dropped k-tile at a piece boundary, swapped segment operands, a shifted output, a skipped bias, an ignored beta, a C read at
beta == 0, a neighbour graph's B and a written canary on every case they apply to).

Yardstick (derived in tests/gemm_ref.py, nothing measured in it): |got - want| <= (Ktot + 16) * 2**-24 * terms with terms =
|alpha| sum |a||b| + |bias| + |beta||C0| of that element and Ktot its reduction length (extra segments included; ragged 2: the graph's
own K; ragged 3: the chunk's); exactly zero where terms is zero; nothing non-finite.  An excess is the largest ratio of an error to that
allowance; every one must be <= 1, and is printed per case and kernel.  Every case runs on two input families: 'ints' (operands in
{-3..3}, bias and C0 in {-8..8}: the result must EQUAL the reference) and 'reals' (magnitudes in [1, 1.25), random signs: the
allowance, and the recorded bar that the rms of err / terms stays below twice that of a sequential float32 chain on the same inputs,
computed on the CPU, plus 2**-30 -- both rms values are printed).

Operands sit in NaN-filled allocations (row padding, gaps between batch items, the floats in front of a misaligned base), C in a
canary-filled one with padding columns, gaps and spare rows; a C that beta == 0 must not read starts as NaN.  Each launch runs twice
on fresh buffers, with containment asserted both times and identical bits (the fixed summation order of the tail split).  The route is
forced with cgc_gemm_tuning and HipKernels.tail_split inside try / finally.

Which case reaches which instance (tile shapes 1..6 = 128x128, 128x64, 64x128, 64x64, 128x32, 32x128; <lay> = NN / NT / TN; the number
behind 'c' is the value given to cgc_gemm_tuning): k_gemm_f32<FAST> on tile t: A-c1t-<lay>-K180/K181/K183-fit, -ldcodd and -misC (scalar
epilogue over the whole tile), -ldcodd-split (the same through k_gemm_fixup); k_gemm_f32<!FAST>: A-c1t-<lay>-K181-odd (both operands
through load), -K183-misA and -K181-misB (one operand through load, the other through load_fast / load_fast_masked);
k_gemm_f32_shortk: A-c2t-<lay>-K41-* and -K1-*.  The full table is at the top of tests/gemm_ref.py (A-*: every instance; B-*: K
remainders; C-*: tail split and fix-up; D-*: TileMap modes; E-*: ragged = 3 and cgc_reduce_batched over its parts; F-*: extra segments;
G-*: degenerate and invalid calls); every case's ``route`` names the kernel instance, TileMap mode, L and S it is expected to reach.
test_one_product_on_every_instance is H, test_reduce_kernels is I.  Out of scope: the >= 4 GiB operand limits of gemm_all_fast
(operands too large for a quick test).

Measured on an MI355X when the suite was first run (all 498 cases equal on 'ints'), the largest excess on 'reals' per kernel kind:
k_gemm_f32<FAST> 0.108 (D-raggedK-TN-nb72), k_gemm_f32<!FAST> 0.099 (B-c11-NN-K8-odd), k_gemm_f32_shortk 0.093 (B-c24-NN-K7-fit); through
k_gemm_fixup: FAST pieces 0.057 (C-raggedK-TN), guarded pieces 0.012 (F-flat-NN-x24+33-xodd); cgc_reduce_batched over the parts of ragged 3:
0.0016; the reduce kernels: k_reduce_batch_sum 0.33, k_reduce_many_parts 0.33 (both at parts = 1, where the allowance is 3 units).  The
largest ratio of the kernel's rms of err / terms to the sequential float32 chain's: 1.02 (B-c25-NT-K73-fit; the bar is 2; on most cases
0.95 .. 1.0, on the long reductions cut by the tail split down to 0.31 at S = 12).  H: all 12 + 18 instances of each layout gave equal
values."""
import contextlib

import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
import gemm_ref as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


@contextlib.contextmanager
def forced(k, cfg, split, mode=0):
    old = k.lib.cgc_gemm_tuning(cfg)
    try:
        k.tail_split, k.gemm_mode = split, mode
        yield
    finally:
        k.tail_split, k.gemm_mode = True, kernels.GEMM_EXACT
        k.lib.cgc_gemm_tuning(old)


def twice(run):
    """run(Places) -> output buffer, twice on fresh buffers: containment both times, identical bits."""
    first, second = G.Places(DEV), G.Places(DEV)
    o1, o2 = run(first), run(second)
    torch.cuda.synchronize()
    first.check(), second.check()
    assert G.same_bits(o1.t, o2.t), 'the second launch differs from the first'
    return o1


@pytest.mark.parametrize('case', G.VALID, ids=lambda c: c.name)
def test_gemm(case):
    k = hip()
    with forced(k, case.cfg, case.split):
        ex, res = G.check_case(k, case, twice, with_chain=True)
        red = {}
        if case.ragged == 3:
            for fam in ('ints', 'reals'):
                P = G.Places(DEV)
                red[fam] = G.reduce_parts_check(k, P, case, res[fam].buf, fam)
                P.check()
    r, rt = res['reals'], case.route
    print('GEMM %s [tile %d %s %s mode %d L %d S %d]: %s rms=%.3g chain=%.3g ratio=%.3g%s' % (
        case.name, rt.tile, rt.kernel, rt.lay, rt.mode, rt.L, rt.S, ex.line(), r.rms, r.chain, r.rms / max(r.chain, G.RMS_FLOOR),
        ''.join(' reduce-%s=%.3g' % kv for kv in sorted(red.items()))))
    assert res['ints'].equal and res['ints'].excess == 0.0, '%s: ints differ from the reference' % case.name
    assert r.excess <= 1.0, '%s: error above the allowance: %r' % (case.name, ex)
    assert r.rms <= G.RMS_FACTOR * r.chain + G.RMS_FLOOR, '%s: rms %g above twice the chain\'s %g' % (case.name, r.rms, r.chain)
    assert all(e <= 1.0 for e in red.values()), red


@pytest.mark.parametrize('case', [c for c in G.CASES if c.expect != 'ok'], ids=lambda c: c.name)
def test_gemm_refuses_or_skips_without_writing(case):
    """N = 0, batch = 0 and M = 0 return 0; every CGC_EINVAL condition raises; neither writes a byte of C."""
    k = hip()
    d = G.data(case, 'ints')
    P = G.Places(DEV)
    with forced(k, case.cfg, case.split, case.over.get('mode', 0)):
        if case.expect == 'einval':
            with pytest.raises(RuntimeError, match='cgc_gemm_f32 failed'):
                G.run(k, P, case, d)
        else:
            G.run(k, P, case, d)
        torch.cuda.synchronize()
    assert len(P.watch) == 1 and G.same_bits(P.watch[0].t, P.watch[0].before)


@pytest.mark.parametrize('lay', list(G.LAYOUTS))
def test_one_product_on_every_instance(lay):
    """H: M = 165, N = 149, K = 181 with an extra segment of 24 ('x') and without ('plain'), tail split off.  An element's k order is
    the same in every instance -- k-tiles in sequence, groups of 8, the pair {8kb+t, 8kb+4+t}; a skipped group only adds 0 * 0 -- so
    the six tile shapes x {FAST, guarded} (and the short-K kernel on the plain product) must give EQUAL values."""
    k = hip()
    outs = {'x': {}, 'plain': {}}
    for prod, case in G.h_cases(lay):
        with forced(k, case.cfg, case.split):
            ex, res = G.check_case(k, case, twice, families=('reals',))
        assert res['reals'].excess <= 1.0, (case.name, ex)
        outs[prod][case.name] = res['reals'].outs[0]
    assert len(outs['x']) == 12 and len(outs['plain']) == 18
    for prod, o in outs.items():
        first = sorted(o)[0]
        differ = [name for name in sorted(o) if not torch.equal(o[name], o[first])]
        print('GEMM H %s %s: %d instances, differing from %s: %r' % (lay, prod, len(o), first, differ))
        assert not differ, differ


@pytest.mark.parametrize('parts', G.REDUCE_PARTS)
def test_reduce_kernels(parts):
    """I: cgc_reduce_batch_sum (k_reduce_batch_sum below 16 parts, k_reduce_many_parts from 16) and cgc_reduce_batched: 'ints' equal,
    'reals' within (parts + 2) * 2**-24 * terms; out in a canary-filled buffer, NaN where beta == 0; repeat runs bitwise identical."""
    k = hip()
    ex = G.Excess()
    for numel in G.REDUCE_NUMEL:
        for outer in G.REDUCE_OUTER:
            for beta in G.REDUCE_BETA:
                for fam in ('ints', 'reals'):
                    r = G.reduce_inputs(fam, parts, numel, outer, beta)
                    for entry in ('batched',) + (('sum',) if outer == 1 else ()):
                        o = twice(lambda P: G.run_reduce(k, P, r, entry, parts, numel, outer, beta))
                        e = G.judge_reduce(fam, r, parts, G.Places.items_of(o)[0])
                        ex.add('%s %s' % (G.reduce_kernel(entry, parts), fam), e)
                        assert e <= 1.0, (parts, numel, outer, beta, fam, entry, e)
    print('GEMM reduce parts=%d: %s' % (parts, ex.line()))
