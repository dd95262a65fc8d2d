"""GPU: the max readout (csrc/rowops.hip: k_segment_max_fwd, k_segment_max_bwd, k_segment_max_bwd_full) against the exact reference
of tests/segmax_ref.py: bits of out, equality of arg, bits of dx.  tests/test_segmax_ref_cpu.py asserts that the cases reach every
lane layout (dp 2 .. 64), both scans and every column group, that the prescribed columns sit where their names say, and that every
mutant -- a NaN ignored and an all -inf column taken for an empty graph among them, which is what k_segment_max_fwd did before these
tests -- is rejected.

Per case (one width, one variant of the prescribed columns, nmax = the longest graph or one more): the forward into canary-surrounded
out and arg; both backward kernels over the reference's arg plane and over that plane with a whole column and a whole graph set to -1,
cgc_segment_max_bwd into a zeroed buffer, cgc_segment_max_bwd_full into a NaN-filled one whose rows before gptr[0] and after gptr[B]
must keep the canary.  Everything runs twice on fresh buffers, aligned and one float past a 16-byte boundary, with identical bits.

With the kernel as it was before the NaN and -inf rules (strict `v > best` from best = -inf, idx = -1), 47 of the 122 forward cases
fail, and only in the columns nan_one, nan_two, nan_after_inf and nan_all (padded or not) and in neginf_all of the one unpadded
graph; every other (graph, column) and every backward case gives the same bits as now."""
import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, ops
import segmax_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def twice(run):
    """run(Place) -> tuple of numpy arrays, on an aligned and on a misaligned placement: containment both times, identical bits."""
    first, second = S.Place(DEV, 'aligned'), S.Place(DEV, 'misaligned')
    o1, o2 = run(first), run(second)
    first.check(), second.check()
    for a, b in zip(o1, o2):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), 'the second launch differs from the first'
    return o1


@pytest.mark.parametrize('case', S.CASES, ids=lambda c: c.name)
def test_forward(case):
    out, arg = twice(lambda P: S.run_forward(hip(), P, case))
    bad = S.judge_forward(case, out, arg)
    assert not bad, '%s: %d wrong (graph, column, prescription), first %r' % (case.name, len(bad), bad[:6])


@pytest.mark.parametrize('case', S.CASES, ids=lambda c: c.name)
def test_backward(case):
    _, arg = S.reference(case)
    for plane in (arg, S.masked_arg(arg)):
        dx, full = twice(lambda P: S.run_backward(hip(), P, case, plane))
        want, want_full = S.backward_reference(case, plane)
        assert S.same_bits(dx, want), '%s: cgc_segment_max_bwd' % case.name
        assert S.same_bits(full, want_full), '%s: cgc_segment_max_bwd_full' % case.name


def test_autograd_matches_float64_max_over_the_padded_tensor():
    """ops.segment_max forward and backward against torch.max over the dense padded tensor in float64, on data without ties."""
    counts, D, nmax = (5, 0, 70, 33), 20, 71
    gptr = torch.tensor(np.cumsum((0,) + counts), dtype=torch.int32)
    rs = np.random.RandomState(7)
    x = torch.from_numpy(rs.standard_normal((sum(counts), D)).astype(np.float32))
    x[5:75, 0] = -x[5:75, 0].abs() - 0.5                          # the padding wins a column
    w = torch.from_numpy(rs.standard_normal((len(counts), D)).astype(np.float32))
    xd = x.to(DEV).requires_grad_(True)
    out = ops.segment_max(xd, gptr.to(DEV), len(counts), nmax)
    (out * w.to(DEV)).sum().backward()
    x64 = x.double().requires_grad_(True)
    dense = torch.stack([torch.cat([x64[int(gptr[b]):int(gptr[b + 1])], torch.zeros(nmax - c, D, dtype=torch.float64)])
                         for b, c in enumerate(counts)])
    ref = dense.max(dim=1).values
    (ref * w.double()).sum().backward()
    assert torch.equal(out.detach().cpu().double(), ref.detach())
    assert torch.equal(xd.grad.cpu().double(), x64.grad)
