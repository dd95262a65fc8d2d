"""CPU: the float64 reference of tests/rowops_ref.py against independent forms (torch.softmax, F.batch_norm, the unfused composition
of the adjacency transforms), the margins of every input of tests/test_rowops_fp64_gpu.py to every decision (clamp at 1, zero
off-diagonal sum, activation kink), and the float32 twin (oracle/flat_ref.TorchKernels) on those inputs under the two yardsticks of
the GPU file.  e32, the twin's excess, is held to 0.25; an output that cannot meet that in float32 would carry its measured e32 in
the table E32 below, and the GPU bound of that output at that width would become max(1, 4 * e32).

    family      output      width    e32
    (none: the largest e32 over all cases is 0.16, the softmax probabilities at 2047 columns; y stays below 0.1, everything
     else below 0.04 -- so every GPU bound is 1)

The inputs are built for that: the BatchNorm shift lies outside the range of the scaled activations (rowops_ref.outside_beta) and the
conv outputs have mean 1, so that neither y nor a column's mean cancels; judged purely relative, a cancelling y or mean would put
the float32 twin itself hundreds of times above the yardstick at whichever element happens to cancel best."""
import pytest
import torch

import rowops_ref as R
from oracle.flat_ref import TorchKernels

# (family, output, width) -> e32 of the float32 twin, the largest over the row counts of that width; absent: e32 <= 0.25
E32 = {
}


def bound(family, name, width):
    """The bound of a GPU excess: 1, or 4 x the float32 twin's own excess where the table above records one."""
    return max(1.0, 4.0 * E32.get((family, name, width), 0.0))


TWIN = TorchKernels()
EPILOGUE_CASES = R.row_cases() + [(w, R.N_BASE) for w in R.FORCED_WIDTHS if (w, R.N_BASE) not in R.row_cases()]
SOFTMAX_CASES = EPILOGUE_CASES + [(w, R.N_BASE) for w in R.BEYOND_WIDTHS]
ADJ_WIDTHS = tuple(sorted(set(R.VEC_WIDTHS + R.SCALAR_WIDTHS + R.FORCED_WIDTHS + R.BEYOND_WIDTHS)))


# ---------------------------------------------------------------------------------------------- reference against independent forms
@pytest.mark.parametrize('C', [4, 18, 114])
def test_reference_softmax_is_torch_softmax(C):
    c = R.softmax_inputs(C, 37)
    want = torch.softmax(c.x.double(), dim=1)
    got = R.softmax_fwd(c.x, 37, C)
    assert float((got - want).abs().max()) <= 1e-15
    x = c.x.double().requires_grad_()
    dx, = torch.autograd.grad(torch.softmax(x, dim=1), [x], c.dS.double())
    ref = R.softmax_bwd(c.x, c.dS, 37, C)
    assert float((ref.dx - dx).abs().max()) <= 1e-14 * float(dx.abs().max())
    assert bool((ref.dx_terms >= ref.dx.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('F', [4, 18, 114])
@pytest.mark.parametrize('extra', [0, 17])
def test_reference_batchnorm_is_torch_batch_norm(F, extra):
    """bn_finalize + bn_act_apply on `count` = n + extra rows are F.batch_norm over the activations followed by `extra` zero rows,
    running statistics included; the backward of epilogue() is autograd through F.batch_norm on the padded rows."""
    n = 37
    c = R.epilogue_inputs(F, n)
    count = float(n + extra)
    act = 2
    st = R.l2norm_act_stats(c.h, n, F, True, act)
    beta = 0.3 * c.mean_run.double() / 0.05
    rm0, rv0 = 0.1 * beta, 1.0 + c.gamma.double()
    fin = R.bn_finalize(st.stats, count, R.BN_EPS, R.MOMENTUM, rm0, rv0)
    y = R.bn_act_apply(st.hn, n, F, act, fin.mean, fin.istd, c.gamma, beta)
    eps, mom = float(torch.tensor(R.BN_EPS, dtype=torch.float32)), float(torch.tensor(R.MOMENTUM, dtype=torch.float32))
    h = c.h.double().requires_grad_()
    o = torch.nn.functional.elu(torch.nn.functional.normalize(h, dim=1))
    padded = torch.cat([o, torch.zeros(extra, F, dtype=torch.float64)])
    rm, rv = rm0.clone(), rv0.clone()
    want = torch.nn.functional.batch_norm(padded, rm, rv, c.gamma.double(), beta, True, mom, eps)[:n]
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(y, want.detach()) and close(fin.running_mean, rm) and close(fin.running_var, rv)
    dh, = torch.autograd.grad(want, [h], c.dy.double())
    ref = R.epilogue(c.h, c.dy, n, F, act, True, 2, count, c.gamma, beta)
    keep = torch.ones(n, dtype=torch.bool)
    keep[c.zero_row] = False              # F.normalize's own gradient at the zero row is judged in the GPU file, against the clamp
    assert close(ref.y, want.detach()) and close(ref.dh[keep], dh[keep])
    assert bool((ref.dh_terms[keep] >= ref.dh[keep].abs() * (1 - 1e-9)).all())
    assert ref.zero_rows == [c.zero_row] and float(ref.rinv[c.zero_row]) == 1e12


@pytest.mark.parametrize('C', [4, 18, 114])
def test_reference_adjacency_is_the_unfused_composition(C):
    """adj_prep = dense_renorm then dense_rownorm, forward and backward; the re-normalisation is _re_norm_adj written on [B, C, C]."""
    c = R.adjacency_inputs(C)
    A3 = c.A.double().clone()
    idx = torch.arange(C)
    A3[:, idx, idx] = 0
    want = A3 / (A3.sum(-1)[..., None] + 1e-15) * (1 - float(torch.tensor(0.4, dtype=torch.float32)))
    want[:, idx, idx] = float(torch.tensor(0.4, dtype=torch.float32))
    re = R.dense_renorm_fwd(c.A, c.R, C, R.P_RENORM)
    assert float((re.out - want.reshape(c.R, C)).abs().max()) <= 1e-15
    rn = R.dense_rownorm_fwd(re.out, c.R, C)
    fused = R.adj_prep_fwd(c.A, c.R, C, R.P_RENORM)
    assert torch.equal(fused.At, re.out) and torch.equal(fused.An, rn.out) and torch.equal(fused.invd, rn.invd)
    for second in (False, True):
        fb = R.adj_prep_bwd(c.A, c.g1, c.g2 if second else None, c.R, C, R.P_RENORM)
        d_at = R.dense_rownorm_bwd(re.out, c.g1, c.R, C).dA + (c.g2.double().reshape(c.R, C) if second else 0.0)
        d_a = R.dense_renorm_bwd(c.A, d_at, c.R, C, R.P_RENORM).dA
        assert float((fb.dA - d_a).abs().max()) <= 1e-12 * float(d_a.abs().max())
        assert bool((fb.dA_terms >= fb.dA.abs() * (1 - 1e-9)).all())
    plain = R.adj_prep_fwd(c.A, c.R, C, None)
    assert plain.At is None and torch.equal(plain.An, R.dense_rownorm_fwd(c.A, c.R, C).out)


# ---------------------------------------------------------------------------------------------- margins of the GPU inputs
def test_inputs_keep_their_distance_from_every_decision():
    for F, n in EPILOGUE_CASES:
        c = R.epilogue_inputs(F, n)
        assert R.margin_epilogue(c) >= R.MARGIN, (F, n)
        if c.zero_row is not None:
            assert float(c.h[c.zero_row].abs().max()) == 0.0
    for C in ADJ_WIDTHS:
        c = R.adjacency_inputs(C)
        clamp, off = R.margin_adjacency(c)
        assert clamp >= R.MARGIN and off >= R.MARGIN, (C, clamp, off)
        # the row sums of the re-normalised adjacency are p + (1-p) s/(s+EPS): 1 by construction, see judge_adjacency
        s = R.adj_prep_fwd(c.A, c.R, C, R.P_RENORM).s
        assert float((s - (1.0 if C > 1 else R.P_RENORM)).abs().max()) <= 1e-7      # (a 1 x 1 adjacency is its diagonal: p)


# ---------------------------------------------------------------------------------------------- the float32 twin
def twin_epilogue(F, n):
    c = R.epilogue_inputs(F, n)
    refs = R.cached('epilogue', F, n, lambda: R.epilogue_reference(c))
    ex = R.Excess()
    for act in R.case_acts(n):
        for nrm in (True, False):
            R.judge_epilogue(c, refs, act, nrm, R.run_epilogue(TWIN, R.Place('cpu'), c, refs, act, nrm), ex)
    return ex


def twin_softmax(C, n):
    c = R.softmax_inputs(C, n)
    ref = R.cached('softmax', C, n, lambda: R.softmax_bwd(c.x, c.dS, n, C))
    ex = R.Excess()
    R.judge_softmax(ref, R.run_softmax(TWIN, R.Place('cpu'), c, ref, beyond=C > 2048), ex)
    return ex


def twin_adjacency(C):
    c = R.adjacency_inputs(C)
    ref = R.cached('adjacency', C, 0, lambda: R.adjacency_reference(c))
    ex = R.Excess()
    R.judge_adjacency(ref, R.run_adjacency(TWIN, R.Place('cpu'), c, ref), ex)
    return ex


def _hold(family, width, ex):
    for name, e in ex.items():
        limit = E32.get((family, name, width), 0.25)
        assert e <= limit, '%s %s width %d: e32 = %.3g above %.3g' % (family, name, width, e, limit)


@pytest.mark.parametrize('F,n', EPILOGUE_CASES)
def test_twin_epilogue(F, n):
    _hold('epilogue', F, twin_epilogue(F, n))


@pytest.mark.parametrize('C,n', SOFTMAX_CASES)
def test_twin_softmax(C, n):
    _hold('softmax', C, twin_softmax(C, n))


@pytest.mark.parametrize('C', ADJ_WIDTHS)
def test_twin_adjacency(C):
    _hold('adjacency', C, twin_adjacency(C))
