"""Float64 reference of the row kernels (csrc/rowops.hip) for tests/test_rowops_ref_cpu.py and tests/test_rowops_fp64_gpu.py, written
from the contracts in include/cgc_hip.h and the layers they cite -- F.normalize (x / max(||x||_2, 1e-12)), the activations of
model/network.py:84-91, nn.BatchNorm1d over `count` rows (model/network.py:101-107), torch.softmax (model/network.py:200),
_re_norm_adj (model/network.py:183-191, EPS = 1e-15) and DenseSAGEConv's adj / adj.sum(-1).clamp(min=1) -- independent of
oracle/flat_ref.py.  Every backward is torch.autograd.grad through the float64 forward.  Beside each output that is a sum of
mixed-sign terms the reference returns ``terms``: the sum of the absolute values of its summands, the base of the absolute tolerance.

Beside the operators: the inputs the GPU tests run (shared with the CPU tests, which pin the float32 twin on them and assert the
margins to every decision), the call sequences (``run_*``: the same code drives the float32 twin on the CPU and the HIP kernels), and
the two yardsticks (``judge_*``)."""
import numpy as np
import torch

from util import elementwise_excess

L2_EPS = 1e-12
RENORM_EPS = 1e-15
BN_EPS = 1e-5
MOMENTUM = 0.1
P_RENORM = 0.4
RTOL_POINT = 1e-5            # the project's softmax figure, applied per element
RTOL_SUM = 1e-4              # the project's float32 figure (TOL), times the sum of |summands|
ATOL_SUM = 1e-7
MARGIN = 1e-3
CANARY = 1234.5

# One width per (VEC, MAXJ, lpr) class of col_cfg(); 20 and 516 are the forced-scalar widths; 2049 / 2052 lie beyond the envelope.
VEC_WIDTHS = (4, 32, 36, 68, 132, 256, 260, 516, 1028, 1140, 1284, 2048)
SCALAR_WIDTHS = (1, 7, 13, 18, 33, 63, 65, 129, 257, 513, 1025, 2047)
FORCED_WIDTHS = (20, 516)
BEYOND_WIDTHS = (2049, 2052)
N_BASE = 37                  # leaves a partly filled last wave at every lanes-per-row count
# lanes per row -> (a row count with >= 129 slots, one just past MAX_SLOTS = 1024 workgroups): row_blocks() of common.hpp gives
# 4 * (64 / lpr) rows per workgroup
GRID_ROWS = {64: (530, 4100), 32: (1060, 8200), 16: (2120, 16400), 8: (4200, 32800)}
GRID_WIDTHS = {32: 8, 36: 16, 68: 32, 132: 64, 7: 8, 13: 16, 18: 32, 33: 64}      # width -> lanes per row


def row_cases():
    """(width, n) of every aligned case of the row kernels (epilogue and softmax)."""
    out = [(w, N_BASE) for w in VEC_WIDTHS + SCALAR_WIDTHS]
    for w, lpr in GRID_WIDTHS.items():
        out += [(w, 1), (w, GRID_ROWS[lpr][0]), (w, GRID_ROWS[lpr][1])]
    return out


def adj_batch(C):
    """B of the [B, C, C] adjacency: R = B * C is no multiple of the rows of a wave where some B allows that."""
    return 3 if C <= 132 else 2 if C < 1025 else 1


class Bag(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _d(t):
    return None if t is None else t.detach().double().cpu().clone()


def _put(out, val):
    if out is not None:
        out.copy_(val.to(out.dtype))


def f32(t):
    """The float32 rounding of a float64 reference value: what the test hands a kernel that consumes a saved forward output."""
    return None if t is None else t.detach().float()


# ------------------------------------------------------------------------------------------------ operators in float64
def activation(x, act):
    if act == 0:
        return x
    if act == 1:
        return torch.relu(x)
    if act == 2:
        return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0.0)))
    if act == 3:
        return torch.where(x > 0, x, 0.01 * x)
    raise ValueError(act)


def _l2norm(h, normalize):
    if not normalize:
        return h, torch.ones(h.shape[0], dtype=h.dtype)
    rinv = 1.0 / torch.linalg.vector_norm(h, dim=1).clamp(min=L2_EPS)
    return h * rinv.unsqueeze(1), rinv


def l2norm_act_stats(h, n, F, normalize, act, hn_out=None, rinv_out=None, stats_out=None):
    """-> Bag(hn, rinv, stats [2,F], terms [2,F], zero_rows): rows whose norm is below the clamp carry rinv = 1e12."""
    h = _d(h)[:n, :F]
    hn, rinv = _l2norm(h, normalize)
    o = activation(hn, act)
    stats = torch.stack([o.sum(0), (o * o).sum(0)])
    terms = torch.stack([o.abs().sum(0), (o * o).sum(0)])
    zero_rows = torch.nonzero(torch.linalg.vector_norm(h, dim=1) < L2_EPS).flatten().tolist() if normalize else []
    _put(hn_out, hn), _put(rinv_out, rinv), _put(stats_out, stats)
    return Bag(hn=hn, rinv=rinv, stats=stats, terms=terms, zero_rows=zero_rows)


def bn_finalize(stats, count, eps, momentum, running_mean, running_var, mean_out=None, istd_out=None):
    """-> Bag(mean, istd, var, running_mean, running_var); eps and momentum are the C floats of the entry point."""
    stats = _d(stats)
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    mean = stats[0] / count
    var = stats[1] / count - mean * mean
    istd = 1.0 / torch.sqrt(var + eps)
    rm = rv = None
    if running_mean is not None:
        rm = (1.0 - momentum) * _d(running_mean) + momentum * mean
        rv = (1.0 - momentum) * _d(running_var) + momentum * var * count / (count - 1.0)
    _put(mean_out, mean), _put(istd_out, istd)
    return Bag(mean=mean, istd=istd, var=var, running_mean=rm, running_var=rv)


def l2norm_act_bn(h, n, F, normalize, act, hn_out, rinv_out, count, eps, momentum, running_mean, running_var, num_batches_tracked,
                  mean_out, istd_out):
    a = l2norm_act_stats(h, n, F, normalize, act, hn_out, rinv_out)
    b = bn_finalize(a.stats, count, eps, momentum, running_mean, running_var, mean_out, istd_out)
    nbt = None if num_batches_tracked is None else int(num_batches_tracked) + 1
    return Bag(hn=a.hn, rinv=a.rinv, stats=a.stats, mean=b.mean, istd=b.istd, running_mean=b.running_mean,
               running_var=b.running_var, num_batches_tracked=nbt, zero_rows=a.zero_rows)


def bn_act_apply(hn, n, F, act, mean, istd, gamma, beta, y_out=None, ldy=None):
    o = activation(_d(hn)[:n, :F], act)
    y = o if mean is None else (o - _d(mean)) * _d(istd) * _d(gamma) + _d(beta)
    if y_out is not None:
        y_out[:n, :F].copy_(y.to(y_out.dtype))
    return y


def colsum(x, ld, n, F, out=None):
    x = _d(x)[:n, :F]
    r = Bag(out=x.sum(0), terms=x.abs().sum(0))
    _put(out, r.out)
    return r


def _softmax(x):
    e = torch.exp(x - x.max(dim=1, keepdim=True).values.detach())
    return e / e.sum(1, keepdim=True)


def softmax_fwd(x, n, C, out=None, ld=None):
    S = _softmax(_d(x)[:n, :C])
    if out is not None:
        out[:n, :C].copy_(S.to(out.dtype))
    return S


def _rownorm(A2):
    s = A2.sum(1)
    d = s.clamp(min=1.0)
    return A2 / d.unsqueeze(1), 1.0 / d, (s >= 1.0).to(A2.dtype), s


def _renorm(A2, C, p):
    R = A2.shape[0]
    diag = torch.zeros(R, C, dtype=A2.dtype)
    diag[torch.arange(R), torch.arange(R) % C] = 1.0
    A0 = A2 * (1.0 - diag)
    s = A0.sum(1)
    return (A0 / (s.unsqueeze(1) + RENORM_EPS)) * (1.0 - p) * (1.0 - diag) + p * diag, s, diag


def dense_rownorm_fwd(A, R, C, out=None, invd_out=None, ge1_out=None):
    An, invd, ge1, s = _rownorm(_d(A).reshape(R, C))
    _put(out, An.reshape(out.shape) if out is not None else An), _put(invd_out, invd), _put(ge1_out, ge1)
    return Bag(out=An, invd=invd, ge1=ge1, s=s)


def dense_renorm_fwd(A, R, C, p, out=None):
    At, s, _ = _renorm(_d(A).reshape(R, C), C, float(np.float32(p)))
    _put(out, At.reshape(out.shape) if out is not None else At)
    return Bag(out=At, s_off=s)


def adj_prep_fwd(A, R, C, p, At_out=None, An_out=None, invd_out=None, ge1_out=None):
    A2 = _d(A).reshape(R, C)
    At, s_off = (A2, None) if p is None else _renorm(A2, C, float(np.float32(p)))[:2]
    An, invd, ge1, s = _rownorm(At)
    if p is not None:
        _put(At_out, At.reshape(At_out.shape) if At_out is not None else At)
    _put(An_out, An.reshape(An_out.shape) if An_out is not None else An), _put(invd_out, invd), _put(ge1_out, ge1)
    return Bag(At=(None if p is None else At), An=An, invd=invd, ge1=ge1, s=s, s_off=s_off)


# ------------------------------------------------------------------------------------------------ backward by autograd
def outside_beta(t):
    """A BatchNorm shift that no entry of t [n, F] cancels: beta_f = +-1.25 max_i |t_if| (at least 0.1), the sign alternating with the
    column, rounded to float32.  y = t + beta is judged purely relative per element, which only a y that stays a fixed fraction of
    its two summands can meet in float32; the shift still weighs as much as the scaled activations it is added to."""
    sign = 1.0 - 2.0 * (torch.arange(t.shape[1]) % 2).double()
    return (sign * (1.25 * t.detach().abs().max(0).values).clamp(min=0.1)).float().double()


def epilogue(h, dy, n, F, act, normalize, mode, count, gamma, beta=None, mean_run=None, istd_run=None, eps=BN_EPS):
    """y = BN(act(l2norm(h))) and its backward at the incoming gradient dy, in float64.  mode 2: batch statistics over `count` rows
    (the rows past n are zero padding: they enter the sums as zeros), 1: the given constants mean_run / istd_run, 0: no BN.
    beta None: outside_beta() of the scaled activations, returned as .beta.
    -> Bag: hn, rinv, zero_rows, stats (+ stats_terms), mean, istd, y; sums [2,F] = (sum dy, sum dy * xhat) (+ sums_terms; modes 1, 2);
    dh (+ dh_terms), dhc = column sums of dh (+ dhc_terms)."""
    h = _d(h)[:n, :F].requires_grad_()
    dy = _d(dy)[:n, :F]
    g = _d(gamma).requires_grad_() if mode else None
    hn, rinv = _l2norm(h, normalize)
    o = activation(hn, act)
    stats = torch.stack([o.sum(0), (o * o).sum(0)])
    r = Bag(hn=hn.detach(), rinv=rinv.detach(), stats=stats.detach(),
            stats_terms=torch.stack([o.abs().sum(0), (o * o).sum(0)]).detach(),
            zero_rows=torch.nonzero(torch.linalg.vector_norm(h.detach(), dim=1) < L2_EPS).flatten().tolist() if normalize else [])
    if mode == 2:
        mean = stats[0] / count
        istd = 1.0 / torch.sqrt(stats[1] / count - mean * mean + float(np.float32(eps)))
    elif mode == 1:
        mean, istd = _d(mean_run), _d(istd_run)
    if mode:
        xhat = (o - mean) * istd
        b = (outside_beta(xhat * g) if beta is None else _d(beta)).requires_grad_()
        y = xhat * g + b
        r.beta = b.detach()
        dh, dg, db = torch.autograd.grad(y, [h, g, b], dy)
        r.mean, r.istd = mean.detach(), istd.detach()
        r.sums = torch.stack([db, dg]).detach()
        xh = xhat.detach()
        r.sums_terms = torch.stack([dy.abs().sum(0), (dy * xh).abs().sum(0)])
    else:
        y = o
        dh, = torch.autograd.grad(y, [h], dy)
    r.y, r.dh = y.detach(), dh.detach()
    # magnitudes of the summands of dh: do = gamma istd (dy - s0/count - xhat s1/count), dhn = do act'(hn),
    # dh = rinv (dhn - hn <hn, dhn>) -- only their absolute values; the gradient itself is autograd's
    with torch.no_grad():
        if mode == 2:
            t_do = (g * r.istd).abs() * (dy.abs() + r.sums_terms[0] / count + xh.abs() * r.sums_terms[1] / count)
        elif mode == 1:
            t_do = (g * r.istd).abs() * dy.abs()
        else:
            t_do = dy.abs()
    hd = r.hn.clone().requires_grad_()
    dact, = torch.autograd.grad(activation(hd, act), [hd], torch.ones_like(hd))
    t_dhn = t_do * dact.abs()
    if normalize:
        r.dh_terms = r.rinv.unsqueeze(1) * (t_dhn + r.hn.abs() * (r.hn.abs() * t_dhn).sum(1, keepdim=True))
    else:
        r.dh_terms = t_dhn
    r.dh_terms = r.dh_terms.detach()
    r.dhc, r.dhc_terms = r.dh.sum(0), r.dh_terms.sum(0)
    return r


def softmax_bwd(x, dS, n, C):
    """-> Bag(S, dx, dx_terms, dxc, dxc_terms): dx by autograd through softmax_fwd(x)."""
    x = _d(x)[:n, :C].requires_grad_()
    dS = _d(dS)[:n, :C]
    S = _softmax(x)
    dx, = torch.autograd.grad(S, [x], dS)
    S = S.detach()
    terms = S * (dS.abs() + (dS * S).abs().sum(1, keepdim=True))
    return Bag(S=S, dx=dx.detach(), dx_terms=terms, dxc=dx.detach().sum(0), dxc_terms=terms.sum(0))


def _rownorm_terms(g, An, invd, ge1):
    return invd.unsqueeze(1) * (g.abs() + ge1.unsqueeze(1) * (g * An).abs().sum(1, keepdim=True))


def _renorm_terms(t_dAt, A2, C, p):
    """Summand magnitudes of the re-normalisation backward, q = 1/(s + EPS): dA = (1-p) q (dAt - q <A, dAt>_offdiag) off the diagonal."""
    _, s, diag = _renorm(A2, C, p)
    q = 1.0 / (s + RENORM_EPS)
    A0 = A2 * (1.0 - diag)
    return (1.0 - p) * q.unsqueeze(1) * (t_dAt + q.unsqueeze(1) * (t_dAt * A0).sum(1, keepdim=True)) * (1.0 - diag)


def dense_rownorm_bwd(A, dOut, R, C):
    A2 = _d(A).reshape(R, C).requires_grad_()
    g = _d(dOut).reshape(R, C)
    An, invd, ge1, s = _rownorm(A2)
    dA, = torch.autograd.grad(An, [A2], g)
    return Bag(out=An.detach(), invd=invd.detach(), ge1=ge1.detach(), s=s.detach(), dA=dA.detach(),
               dA_terms=_rownorm_terms(g, An.detach(), invd.detach(), ge1.detach()))


def dense_renorm_bwd(A, dOut, R, C, p):
    p = float(np.float32(p))
    A2 = _d(A).reshape(R, C).requires_grad_()
    g = _d(dOut).reshape(R, C)
    At, s, _ = _renorm(A2, C, p)
    dA, = torch.autograd.grad(At, [A2], g)
    return Bag(out=At.detach(), dA=dA.detach(), dA_terms=_renorm_terms(g.abs(), A2.detach(), C, p), s_off=s.detach())


def adj_prep_bwd(A, gAn, gAt, R, C, p):
    """Backward of adj_prep_fwd at the gradients gAn (of An) and gAt (of At; None: no second stream), by autograd."""
    p = None if p is None else float(np.float32(p))
    A2 = _d(A).reshape(R, C).requires_grad_()
    gn = _d(gAn).reshape(R, C)
    gt = None if gAt is None else _d(gAt).reshape(R, C)
    At = A2 if p is None else _renorm(A2, C, p)[0]
    An, invd, ge1, s = _rownorm(At)
    if gt is None:
        dA, = torch.autograd.grad(An, [A2], gn)
    else:
        dA, = torch.autograd.grad([An, At * 1.0], [A2], [gn, gt])
    t = _rownorm_terms(gn, An.detach(), invd.detach(), ge1.detach())
    if gt is not None:
        t = t + gt.abs()
    if p is not None:
        t = _renorm_terms(t, A2.detach(), C, p)
    return Bag(At=(None if p is None else At.detach()), An=An.detach(), invd=invd.detach(), ge1=ge1.detach(), s=s.detach(),
               dA=dA.detach(), dA_terms=t)


# ------------------------------------------------------------------------------------------------ yardsticks
def excess_point(a, b):
    """Pointwise output: |a-b| <= 1e-5 |b| where the reference is nonzero, exact equality where it is exactly zero."""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    nz = b != 0
    if bool((a[~nz] != 0).any()) or not bool(torch.isfinite(a).all()):
        return float('inf')
    return elementwise_excess(a[nz], b[nz], rtol=RTOL_POINT, atol=0.0)


def excess_sum(a, b, terms):
    """Cancelling sum: |a-b| <= 1e-4 * (sum of |summands|) + 1e-7 per element."""
    a, b, t = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1), terms.double().reshape(-1)
    assert a.shape == b.shape == t.shape, (a.shape, b.shape, t.shape)
    if a.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(a).all()):
        return float('inf')
    return float(((a - b).abs() / (RTOL_SUM * t + ATOL_SUM)).max())


class Excess(dict):
    """name -> the largest excess seen under that name."""
    def add(self, name, e):
        self[name] = max(self.get(name, 0.0), float(e))

    def line(self):
        return ' '.join('%s=%.3g' % kv for kv in sorted(self.items()))


# ------------------------------------------------------------------------------------------------ inputs
def _rnd(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def epilogue_inputs(F, n):
    """h = N(1, 1), so that a column's activations do not cancel in its mean (a sixth of them is negative), and every entry is at
    least 0.01 away from 0 (the activations' kink); row 3 is exactly zero (the clamp of the L2 norm) at n = 37 only: its 1e12
    factor would drown every other row in the fused column sums of the grid-shape cases.  beta is epilogue()'s."""
    h = _rnd(1000 + F, n, F) + 1.0
    h = torch.where(h < 0, -1.0, 1.0) * h.abs().clamp(min=0.01)
    zero_row = 3 if n == N_BASE else None
    if zero_row is not None:
        h[zero_row] = 0.0
    rv = 1.0 + 0.5 * _rnd(5, F).abs()
    return Bag(F=F, n=n, h=h, dy=_rnd(9, n, F), gamma=_rnd(1, F).abs() + 0.5, count=float(n + 17),
               rm0=torch.zeros(F), rv0=torch.ones(F), mean_run=0.05 * _rnd(4, F),
               istd_run=(1.0 / torch.sqrt(rv.double() + float(np.float32(BN_EPS)))).float(), zero_row=zero_row)


def softmax_inputs(C, n):
    return Bag(C=C, n=n, x=_rnd(2000 + C, n, C) * 3, dS=_rnd(1, n, C))


def adjacency_inputs(C):
    """[B, C, C] with positive entries; row sums cycle through 0.3, 1.7 and 3 (away from the clamp at 1), row 1 is the deliberately
    small one.  The off-diagonal sums, which the re-normalisation divides by, follow."""
    B = adj_batch(C)
    A = _rnd(3000 + C, B, C, C).abs().double() + 0.01
    target = torch.tensor([0.3, 1.7, 3.0], dtype=torch.float64)[torch.arange(B * C) % 3].reshape(B, C, 1)
    A = (A / A.sum(-1, keepdim=True) * target).float()
    if C > 1:
        A[0, 1] *= 0.001
    return Bag(C=C, B=B, R=B * C, A=A, g1=_rnd(1, B, C, C), g2=_rnd(2, B, C, C))


def margin_epilogue(c):
    """Smallest |pre-activation| relative to its row's rms, over the rows that are not the deliberate zero row: with and without
    the L2 normalisation the pre-activation is a positive multiple of h."""
    h = c.h.double()
    keep = torch.ones(c.n, dtype=torch.bool)
    if c.zero_row is not None:
        keep[c.zero_row] = False
    h = h[keep]
    return float((h.abs() / h.pow(2).mean(1, keepdim=True).sqrt()).min())


def margin_adjacency(c):
    """(relative distance of every row sum from the clamp at 1, smallest off-diagonal row sum relative to the row sum): the first
    for the inputs the clamped normalisation sees directly; the second keeps the EPS of _re_norm_adj out of the quotient."""
    r = dense_rownorm_fwd(c.A, c.R, c.C)
    s_off = dense_renorm_fwd(c.A, c.R, c.C, P_RENORM).s_off
    return float((r.s - 1.0).abs().min()), (float((s_off / r.s).min()) if c.C > 1 else 1.0)


# ------------------------------------------------------------------------------------------------ placement on a device
class Place(object):
    """How operands reach a device.  variant 'aligned': fresh allocations, row strides that are multiples of 4 where the width is;
    'misaligned': every operand and output is a view one float past a 16-byte boundary; 'ld1': row strides of width + 1 where the
    entry point takes one.  Outputs are carved from canary-filled buffers with two spare rows; ``check()`` asserts that everything
    outside the views still holds the canary bit for bit."""

    def __init__(self, dev, variant='aligned'):
        self.dev, self.variant, self.watch = dev, variant, []
        self.off = 1 if variant == 'misaligned' else 0

    def ld(self, width, pad):
        return width + 1 if self.variant == 'ld1' else width + pad

    def inp(self, t, ld=None):
        """t [rows, width] (or any shape when ld is None) as a view with row stride ld."""
        if t is None:
            return None
        t = t.to(self.dev)
        if ld is None:
            buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=self.dev)
            v = buf[self.off:self.off + t.numel()].view(t.shape)
        else:
            buf = torch.zeros(t.shape[0] * ld + 4, dtype=t.dtype, device=self.dev)
            v = buf[self.off:self.off + t.shape[0] * ld].view(t.shape[0], ld)[:, :t.shape[1]]
        v.copy_(t)
        return v

    def out(self, rows, width=None, ld=None, dtype=torch.float32):
        """Canary-filled output view [rows, width] with row stride ld (contiguous [rows] / [rows, width] when ld is None)."""
        shape = (rows,) if width is None else (rows, width)
        ld = (1 if width is None else width) if ld is None else ld
        total = (rows + 2) * ld + 4
        buf = torch.full((total,), CANARY, dtype=dtype, device=self.dev)
        if width is None:
            v = buf[self.off:self.off + rows]
        else:
            v = buf[self.off:self.off + rows * ld].view(rows, ld)[:, :width]
        mask = torch.ones(total, dtype=torch.bool)
        if width is None:
            mask[self.off:self.off + rows] = False
        else:
            mask[self.off:self.off + rows * ld].view(rows, ld)[:, :width] = False
        self.watch.append((buf, mask))
        return v

    def check(self):
        for buf, mask in self.watch:
            got = buf.cpu()[mask]
            assert torch.equal(got, torch.full_like(got, CANARY)), 'a kernel wrote outside its output'


# ------------------------------------------------------------------------------------------------ call sequences
ACTS = (0, 1, 2, 3)


def case_acts(n):
    """Every activation at n = 37; ReLU and ELU (one with a flat side, one smooth) at the row counts that exist for the grid shape:
    the activation acts per element, whatever the grid."""
    return ACTS if n == N_BASE else (1, 2)


_CACHE = {}


def cached(kind, width, n, make):
    """The float64 reference of a case, computed once per (kind, width, n) and shared by the tests of a module; the few-MB cases of
    the grid shapes are not kept."""
    key = (kind, width, n)
    if key not in _CACHE:
        val = make()
        if width * n > 200000:
            return val
        _CACHE[key] = val
    return _CACHE[key]


def epilogue_reference(c):
    """{(act, normalize, mode): epilogue(...)} of a case, in float64."""
    return {(act, nrm, mode): epilogue(c.h, c.dy, c.n, c.F, act, nrm, mode, c.count, c.gamma, None, c.mean_run, c.istd_run)
            for act in case_acts(c.n) for nrm in (True, False) for mode in (2, 1, 0)}


def run_epilogue(K, P, c, refs, act, nrm):
    """Every entry point of the conv epilogue on kernels K for one activation and one setting of normalize; kernels that consume a
    saved forward output get the float32 rounding of the float64 one.  -> dict name -> tensor."""
    n, F = c.n, c.F
    r2 = refs[(act, nrm, 2)]
    o = {}
    h = P.inp(c.h)
    o['hn'], o['rinv'] = P.out(n, F), P.out(n)
    o['stats'] = P.out(2, F, dtype=torch.float64)
    K.l2norm_act_stats(h, n, F, nrm, act, o['hn'], o['rinv'], o['stats'])
    rm, rv = P.inp(c.rm0), P.inp(c.rv0)
    o['mean'], o['istd'] = P.out(F), P.out(F)
    K.bn_finalize(P.inp(r2.stats), c.count, BN_EPS, MOMENTUM, rm, rv, o['mean'], o['istd'])
    o['rm'], o['rv'] = rm, rv
    rm2, rv2 = P.inp(c.rm0), P.inp(c.rv0)
    nbt = torch.zeros((), dtype=torch.int64, device=P.dev)
    o['f_hn'], o['f_rinv'], o['f_mean'], o['f_istd'] = P.out(n, F), P.out(n), P.out(F), P.out(F)
    K.l2norm_act_bn(h, n, F, nrm, act, o['f_hn'], o['f_rinv'], c.count, BN_EPS, MOMENTUM, rm2, rv2, nbt, o['f_mean'], o['f_istd'])
    o['f_rm'], o['f_rv'], o['nbt'] = rm2, rv2, nbt
    hn32, rinv32 = P.inp(f32(r2.hn)), P.inp(f32(r2.rinv))
    gamma = P.inp(c.gamma)
    ldy = P.ld(F, 4)
    dy = P.inp(c.dy, P.ld(F, 8))
    lddy = dy.stride(0)
    for mode in (2, 1, 0):
        r = refs[(act, nrm, mode)]
        m = str(mode)
        mean32, istd32 = (P.inp(f32(r.mean)), P.inp(f32(r.istd))) if mode else (None, None)
        beta = P.inp(f32(r.beta)) if mode else None
        o['y' + m] = P.out(n, F, ldy)
        K.bn_act_apply(hn32, n, F, act, mean32, istd32, gamma if mode else None, beta, o['y' + m], ldy)
        sums32 = None
        if mode:
            o['sums' + m] = P.out(2, F)
            K.bn_bwd_reduce(dy, lddy, hn32, n, F, act, mean32, istd32, o['sums' + m])
            sums32 = P.inp(f32(r.sums))
        o['dh' + m], o['dhc' + m], o['dhn' + m] = P.out(n, F), P.out(F), P.out(n, F)
        K.bn_act_l2_bwd(dy, lddy, hn32, rinv32, n, F, act, nrm, mode, mean32, istd32, gamma if mode else None, sums32, c.count,
                        o['dh' + m], o['dhc' + m])
        K.bn_act_l2_bwd(dy, lddy, hn32, rinv32, n, F, act, nrm, mode, mean32, istd32, gamma if mode else None, sums32, c.count,
                        o['dhn' + m])
        o['cs_dh' + m] = P.out(F)
        K.colsum(o['dh' + m], F, n, F, o['cs_dh' + m])
    o['cs_dy'] = P.out(F)
    K.colsum(dy, lddy, n, F, o['cs_dy'])
    return o


def judge_epilogue(c, refs, act, nrm, o, ex):
    """Adds the excesses of run_epilogue's outputs to ``ex``.  The clamped zero row of dh is judged under its own name."""
    r2 = refs[(act, nrm, 2)]
    fin = bn_finalize(r2.stats, c.count, BN_EPS, MOMENTUM, c.rm0, c.rv0)
    for pre in ('', 'f_'):
        ex.add('hn', excess_point(o[pre + 'hn'], r2.hn))
        ex.add('rinv', excess_point(o[pre + 'rinv'], r2.rinv))
        ex.add('mean', excess_point(o[pre + 'mean'], fin.mean))
        ex.add('istd', excess_point(o[pre + 'istd'], fin.istd))
        ex.add('running_mean', excess_point(o[pre + 'rm'], fin.running_mean))
        ex.add('running_var', excess_point(o[pre + 'rv'], fin.running_var))
    ex.add('stats', excess_sum(o['stats'], r2.stats, r2.stats_terms))
    assert int(o['nbt'].item()) == 1
    keep = torch.ones(c.n, dtype=torch.bool)
    if nrm and c.zero_row is not None:
        keep[c.zero_row] = False
    for mode in (2, 1, 0):
        r, m = refs[(act, nrm, mode)], str(mode)
        ex.add('y', excess_point(o['y' + m], r.y))
        if mode:
            ex.add('sums', excess_sum(o['sums' + m], r.sums, r.sums_terms))
        dh = o['dh' + m].detach().cpu()
        ex.add('dh', excess_sum(dh[keep], r.dh[keep], r.dh_terms[keep]))
        if not bool(keep.all()):
            ex.add('dh_zero_row', excess_sum(dh[~keep], r.dh[~keep], r.dh_terms[~keep]))
        ex.add('dhc', excess_sum(o['dhc' + m], r.dhc, r.dhc_terms))
        ex.add('colsum', excess_sum(o['cs_dh' + m], r.dhc, r.dhc_terms))
    cs = colsum(c.dy, c.F, c.n, c.F)
    ex.add('colsum', excess_sum(o['cs_dy'], cs.out, cs.terms))


def run_softmax(K, P, c, ref, beyond=False):
    n, C = c.n, c.C
    ld = P.ld(C, 4)
    x = P.inp(c.x, ld)
    o = {'S': P.out(n, C, ld)}
    K.softmax_fwd(x, n, C, o['S'], ld)
    o['S_inplace'] = P.out(n, C, ld)
    o['S_inplace'].copy_(x)
    K.softmax_fwd(o['S_inplace'], n, C, o['S_inplace'], ld)
    if beyond:
        return o
    S32, dS = P.inp(f32(ref.S), ld), P.inp(c.dS, ld)
    o['dx'], o['dxc'], o['dxn'], o['cs_dx'] = P.out(n, C, ld), P.out(C), P.out(n, C, ld), P.out(C)
    K.softmax_bwd(S32, dS, n, C, o['dx'], o['dxc'], ld)
    K.softmax_bwd(S32, dS, n, C, o['dxn'], None, ld)
    K.colsum(o['dx'], ld, n, C, o['cs_dx'])
    return o


def judge_softmax(ref, o, ex):
    ex.add('softmax', excess_point(o['S'], ref.S))
    ex.add('softmax', excess_point(o['S_inplace'], ref.S))
    if 'dx' in o:
        ex.add('softmax_dx', excess_sum(o['dx'], ref.dx, ref.dx_terms))
        ex.add('softmax_dxc', excess_sum(o['dxc'], ref.dxc, ref.dxc_terms))
        ex.add('colsum', excess_sum(o['cs_dx'], ref.dxc, ref.dxc_terms))


def adjacency_reference(c):
    r = Bag(rownorm=dense_rownorm_bwd(c.A, c.g1, c.R, c.C), renorm=dense_renorm_bwd(c.A, c.g1, c.R, c.C, P_RENORM), prep={})
    for p in (None, P_RENORM):
        for second in (False, True):
            r.prep[(p, second)] = adj_prep_bwd(c.A, c.g1, c.g2 if second else None, c.R, c.C, p)
    return r


def run_adjacency(K, P, c, ref):
    R, C = c.R, c.C
    A, g1, g2 = P.inp(c.A.reshape(R, C)), P.inp(c.g1.reshape(R, C)), P.inp(c.g2.reshape(R, C))
    o = {'rn_out': P.out(R, C), 'rn_invd': P.out(R), 'rn_ge1': P.out(R), 'rn_dA': P.out(R, C), 're_out': P.out(R, C),
         're_dA': P.out(R, C)}
    K.dense_rownorm_fwd(A, R, C, o['rn_out'], o['rn_invd'], o['rn_ge1'])
    rr = ref.rownorm
    K.dense_rownorm_bwd(g1, P.inp(f32(rr.out)), P.inp(f32(rr.invd)), P.inp(f32(rr.ge1)), R, C, o['rn_dA'])
    K.dense_renorm_fwd(A, R, C, P_RENORM, o['re_out'])
    K.dense_renorm_bwd(A, g1, R, C, P_RENORM, o['re_dA'])
    for p in (None, P_RENORM):
        tag = 'n' if p is None else 'p'
        rp = ref.prep[(p, False)]
        if p is not None:
            o['At_' + tag] = P.out(R, C)
        o['An_' + tag], o['invd_' + tag], o['ge1_' + tag] = P.out(R, C), P.out(R), P.out(R)
        K.adj_prep_fwd(A, R, C, p, o.get('At_' + tag), o['An_' + tag], o['invd_' + tag], o['ge1_' + tag])
        An32, invd32, ge132 = P.inp(f32(rp.An)), P.inp(f32(rp.invd)), P.inp(f32(rp.ge1))
        for second in (False, True):
            key = 'dA_%s%d' % (tag, second)
            o[key] = P.out(R, C)
            K.adj_prep_bwd(A, An32, invd32, ge132, g1, g2 if second else None, R, C, p, o[key])
    return o


def judge_adjacency(ref, o, ex):
    """ge1 of the fused pass with re-normalisation is not judged: the row sums of a re-normalised adjacency are 1 up to rounding by
    construction (p + (1-p) s/(s+EPS)), so that flag is decided by the last bit; the backward is handed the reference's flag, and dA
    does not depend on it beyond rounding (the row sum it differentiates is constant)."""
    rr, re = ref.rownorm, ref.renorm
    ex.add('An', excess_point(o['rn_out'], rr.out))
    ex.add('invd', excess_point(o['rn_invd'], rr.invd))
    ex.add('ge1', 0.0 if torch.equal(o['rn_ge1'].cpu().double(), rr.ge1) else float('inf'))
    ex.add('rownorm_dA', excess_sum(o['rn_dA'], rr.dA, rr.dA_terms))
    ex.add('renorm', excess_point(o['re_out'], re.out))
    ex.add('renorm_dA', excess_sum(o['re_dA'], re.dA, re.dA_terms))
    for p in (None, P_RENORM):
        tag = 'n' if p is None else 'p'
        rp = ref.prep[(p, False)]
        if p is not None:
            ex.add('At', excess_point(o['At_' + tag], rp.At))
        else:
            ex.add('ge1', 0.0 if torch.equal(o['ge1_' + tag].cpu().double(), rp.ge1) else float('inf'))
        ex.add('An', excess_point(o['An_' + tag], rp.An))
        ex.add('invd', excess_point(o['invd_' + tag], rp.invd))
        for second in (False, True):
            r = ref.prep[(p, second)]
            ex.add('prep_dA', excess_sum(o['dA_%s%d' % (tag, second)], r.dA, r.dA_terms))
