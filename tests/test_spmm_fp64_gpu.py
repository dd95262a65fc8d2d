"""GPU: the gather kernels of csrc/spmm.hip (k_spmm<4>, k_spmm<1>, k_spmm_wide) against the float64 reference of tests/spmm_ref.py,
element by element, on every kernel instance and every branch of the block-id arithmetic that launch_gather can select
(tests/test_spmm_ref_cpu.py asserts that the case list reaches them, and that the yardstick notices a dropped or doubled edge, a
wrong weight index, a missing scale and a shifted column tile on every case).

Yardstick (derived in tests/spmm_ref.py, nothing measured in it): |got - want| <= (deg[i] + 4) * 2**-24 * terms[i,j] with terms the
sum of |summands| of that element, exactly zero where terms is zero, nothing non-finite.  An excess is the largest ratio of an error
to that allowance; every one must be <= 1, and is printed.

Per case: the flat entry (cgc_spmm; rows without padding only) and the graph entry (cgc_spmm_graphs), on k_spmm_wide also visit 1, 2
and a caller-supplied gorder.  Row degrees cycle through 0..28, 31, 32, 33, 63, 64, 65, 130; one node of every graph is referenced
by no edge and its row of x is NaN, as are the padding columns of x; out sits in a canary-filled buffer with padding columns and
spare rows.  Each launch runs twice on fresh buffers, with containment asserted both times and identical bits.

Which case reaches what (case names are w<width>-<batch>-<operands>[-ld<stride>][-<operand>mis]; B8 = graphs of 37, 0, 1, 130, 64, 9,
300 and 65 nodes, B16 / B5 = sixteen / five small graphs, n2100 = one graph of 2100 rows with degrees up to 19):

    k_spmm<4>     lpr 8: w4, w32   lpr 16: w36, w64   lpr 32: w68, w128 (the last vector width below k_spmm_wide)
    k_spmm<1>     lpr 8: w1, w3, w7, w4-..-xmis-outmis   lpr 16: w13   lpr 32: w18   lpr 64, one tile: w33, w63, w64-..-xmis-outmis,
                  w64-..-xmis   several tiles: w65 (2), w129 (3), w257, w260-..-xmis-outmis, w260-..-outmis, w260-..-ld261, w300-..-ld301
                  (5 each) -- row chunks on the flat entry, graph chunks on the graph entry; chunk 1 with two tiles: w65-n2100
    k_spmm_wide   one tile: w132, w256   several: w260 (2), w516 (3), w1140 (5); all six <VAL,PERM,PRE> instances with and without
                  post on the flat and on the graph entry: w260-B8-*; order 1 / 2 formula branch: B8 and B16, reversal branch: B5,
                  gorder on each; chunk 1 with two tiles: w260-n2100 (flat)
    every operand combination (twelve, and perm without val with and without pre): w36 (k_spmm<4>), w13 (k_spmm<1>), w260 (wide);
    every other width: val + post (the forward aggregation) and val + perm + pre (its transpose in the backward)
    padded rows: every width once with ld = width + 4; ld = width + 1 at 260 and 300 (scalar kernel, graph chunks)
    tails 0..8 after 0, 1 and 2 full batches of 9, and a second and third staging round at lpr 8, 16, 32 and 64: every B8 case

Measured on an MI355X, the largest excess per kernel over all cases: k_spmm<4> 0.427, k_spmm<1> 0.405, k_spmm_wide 0.463 (the float32
restatement on the CPU: 0.473).  Every launch of a case -- flat, graph, visit 1, 2, gorder -- gave the same excess."""
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
import spmm_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def twice(mis=()):
    """launch(run): run(Places) -> output, twice on fresh buffers: containment both times, identical bits."""
    def launch(run):
        first, second = S.Places(DEV, mis), S.Places(DEV, mis)
        o1, o2 = run(first), run(second)
        torch.cuda.synchronize()
        first.check(), second.check()
        assert same_bits(o1, o2), 'the second launch differs from the first'
        return o1
    return launch


@pytest.mark.parametrize('case', S.CASES, ids=lambda c: c.name)
def test_spmm(case):
    ex, outs = S.check_case(hip(), case, twice(case.mis))
    print('SPMM %s: %s' % (case.name, ex.line()))
    assert ex and len(outs) == len(S.launches(case))
    for tag, o in outs.items():
        assert bool(torch.isfinite(o).all()), '%s %s: non-finite output' % (case.name, tag)
    bad = {k: e for k, e in ex.items() if not e <= 1.0}
    assert not bad, '%s: error above the allowance: %r' % (case.name, bad)


def test_scheduling_does_not_change_a_bit():
    """The arithmetic of a row does not depend on which block computes it: the flat entry, the graph entry, visit 1, 2 and a gorder
    give the same bits (one kernel, k_spmm_wide with two column tiles; no equality is asked across kernels)."""
    case = S.BITS_CASE
    ex, outs = S.check_case(hip(), case, twice())
    assert set(outs) == {'flat', 'graphs', 'visit1', 'visit2', 'gorder'}
    assert {k.split('/')[0] for k in ex} == {'k_spmm_wide'} and all(e <= 1.0 for e in ex.values()), ex
    for tag, o in outs.items():
        assert same_bits(o, outs['flat']), '%s differs from the flat entry' % tag
