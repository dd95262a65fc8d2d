"""Float64 reference of DenseJK (model/network.py:11-55) for the kernel tests of csrc/jk.hip and csrc/jk_mfma.hip, independent of
oracle/flat_ref.py: a manual bidirectional LSTM loop (gate order i, f, g, o) over a node's three layer embeddings, Linear(2H -> 1)
attention, softmax over the three scores, and every gradient by autograd.  Beside it: the inputs the GPU tests run (shared with the
CPU tests that pin the float32 twin on them), weights that make the kernels print their own activation functions, and float32
models of the fast activations that give the readout bound a derivation."""
import functools

import numpy as np
import torch

from util import elementwise_excess

ALL_C = tuple(range(2, 33, 2))
MATRIX_CORE_C = (4, 8, 12, 16, 20)
PARAM_NAMES = ('dW_ih_f', 'dW_hh_f', 'db_ih_f', 'db_hh_f', 'dW_ih_r', 'dW_hh_r', 'db_ih_r', 'db_hh_r', 'dw_att')
ULP = 2.0 ** -23
READOUT_ULPS = 8.0          # bound of the activation readout, in units of 2^-23 relative


class Bag(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---------------------------------------------------------------------------------------------- the operator in float64
def forward(xs, lstm, w_att, b_att):
    """xs [n, 3C]; lstm = (w_ih, w_hh, b_ih, b_hh) forward then reverse; w_att [2H]; b_att [1] -> out [n, C], HS, CS [6H, n]
    (row (d*3 + t)*H + j: direction d, TIME slot t, unit j -- the kernels' layout) and the attention scores [n, 3]."""
    n = xs.shape[0]
    C = xs.shape[1] // 3
    H = 3 * C // 2
    x = xs.reshape(n, 3, C)
    hs = [[None] * 3, [None] * 3]
    cs = [[None] * 3, [None] * 3]
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = lstm[4 * d:4 * d + 4]
        h = xs.new_zeros(n, H)
        c = xs.new_zeros(n, H)
        for s in range(3):
            t = s if d == 0 else 2 - s
            pre = x[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
            i, f = torch.sigmoid(pre[:, 0 * H:1 * H]), torch.sigmoid(pre[:, 1 * H:2 * H])
            g, o = torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:4 * H])
            c = f * c + i * g
            h = o * torch.tanh(c)
            hs[d][t], cs[d][t] = h, c
    score = torch.stack([hs[0][t] @ w_att[:H] + hs[1][t] @ w_att[H:] + b_att[0] for t in range(3)], 1)
    a = torch.softmax(score, dim=1)
    out = (x * a.unsqueeze(-1)).sum(1)
    HS = torch.cat([hs[d][t].t() for d in range(2) for t in range(3)], 0)
    CS = torch.cat([cs[d][t].t() for d in range(2) for t in range(3)], 0)
    return out, HS, CS, score


def reference(xs, lstm, w_att, b_att, dout):
    """Forward and backward in float64.  Returns a Bag: out, HS, CS, score, dxs, grads (ten tensors in split_jk_param_grads order:
    four per direction, d att.weight [1, 2H], d att.bias [1]) and ds [n, 3], the gradient of the attention scores."""
    dd = lambda v: v.detach().double().cpu().clone()
    x = dd(xs).requires_grad_()
    ps = [dd(p).requires_grad_() for p in lstm]
    wa, ba = dd(w_att).reshape(-1).requires_grad_(), dd(b_att).reshape(-1).requires_grad_()
    out, HS, CS, score = forward(x, ps, wa, ba)
    g = torch.autograd.grad(out, [x] + ps + [wa, ba, score], dd(dout))
    H = wa.numel() // 2
    grads = [t.detach() for t in g[1:9]] + [g[9].detach().reshape(1, 2 * H), g[10].detach().reshape(1)]
    return Bag(out=out.detach(), HS=HS.detach(), CS=CS.detach(), score=score.detach(), dxs=g[0].detach(), grads=grads,
               ds=g[11].detach())


def unpack_G(G, C):
    """G [2, 4H+1, C+2H+1] (DGT_d @ INT_d^T, KernelSpec.jk_bwd) -> the ten gradients in split_jk_param_grads order."""
    H = 3 * C // 2
    out = []
    for d in range(2):
        out += [G[d, :4 * H, :C], G[d, :4 * H, C:C + H], G[d, :4 * H, C + H], G[d, :4 * H, C + H]]
    out.append(torch.cat([G[0, 4 * H, C + H + 1:], G[1, 4 * H, C + H + 1:]]).reshape(1, 2 * H))
    out.append(G[0, 4 * H, C + H].reshape(1))
    return out


def tensors(r):
    """(name, tensor) of everything the yardstick is applied to, one entry per tensor (d att.bias is judged apart)."""
    return [('out', r.out), ('HS', r.HS), ('CS', r.CS), ('dxs', r.dxs)] + list(zip(PARAM_NAMES, r.grads[:9]))


def db_att_bound(ref):
    """d att.bias is mathematically zero (the softmax does not see a common shift): its float32 value is the rounding error of a sum
    of the score gradients, which scales with the magnitude of the TERMS."""
    return 1e-4 * float(ref.ds.abs().sum())


# ---------------------------------------------------------------------------------------------- test inputs
# The saturated inputs are a draw of their own.  The plain draw scaled (offset 0) holds, at C = 20, one gate of one x 300 row whose
# pre-activation lands near zero out of terms of several hundred: ANY float32 summation is off by ~1e-4 there or not, depending on
# its order alone (chain_forward: 0.41 ascending, 2.73 in the matrix-core kernels' order, which is to three digits what those
# kernels give; the twin's BLAS order: 0.12).  test_jk_ref_cpu.py holds a draw to 0.25 under every one of these orders; the offset is
# the first multiple of 100000 that meets it for all four channel counts (100000: 0.57 at C = 20).
SATURATED_DRAW = 200000


@functools.lru_cache(maxsize=None)
def case(C, n, kind='plain'):
    """Input of a GPU test, float32 on the CPU (cached: treat as read-only).  Default torch initialisation of nn.LSTM(C, 3C/2) and
    nn.Linear(3C, 1); xs, dout ~ N(0, 1); from 24 rows up, row 3 of xs is zero, rows 8-15 are scaled by 1e-3 (the polynomial branch
    of fast_tanh) and rows 16-23 by 30 (saturated gates in a few rows).  kind 'saturated': LSTM weights x 8 and xs x 10 on top,
    attention unscaled (a draw of its own: SATURATED_DRAW)."""
    H = 3 * C // 2
    gen = torch.Generator().manual_seed(1000 * C + n + (SATURATED_DRAW if kind == 'saturated' else 0))
    k = 1.0 / H ** 0.5
    u = lambda *shape: (torch.rand(*shape, generator=gen) * 2 - 1) * k
    lstm = []
    for _ in range(2):
        lstm += [u(4 * H, C), u(4 * H, H), u(4 * H), u(4 * H)]
    ka = 1.0 / (2 * H) ** 0.5
    w_att = (torch.rand(2 * H, generator=gen) * 2 - 1) * ka
    b_att = (torch.rand(1, generator=gen) * 2 - 1) * ka
    xs = torch.randn(n, 3 * C, generator=gen)
    dout = torch.randn(n, C, generator=gen)
    if n >= 24:
        xs[3] = 0
        xs[8:16] *= 1e-3
        xs[16:24] *= 30
    if kind == 'saturated':
        lstm = [p * 8 for p in lstm]
        xs = xs * 10
    else:
        assert kind == 'plain'
    return Bag(C=C, H=H, n=n, kind=kind, xs=xs, dout=dout, lstm=lstm, w_att=w_att, b_att=b_att)


@functools.lru_cache(maxsize=None)
def case_reference(C, n, kind='plain'):
    c = case(C, n, kind)
    return reference(c.xs, c.lstm, c.w_att, c.b_att, c.dout)


@functools.lru_cache(maxsize=None)
def case_twin(C, n, kind='plain'):
    """The float32 torch twin (oracle/flat_ref.TorchKernels) on the same input, in the shape of ``reference``."""
    from oracle.flat_ref import TorchKernels
    c = case(C, n, kind)
    K, H = TorchKernels(), c.H
    npad = -(-n // 64) * 64
    out = torch.empty(n, C)
    HS, CS = torch.zeros(6 * H, npad), torch.zeros(6 * H, npad)
    K.jk_fwd(c.xs, n, npad, C, c.lstm, c.w_att, c.b_att, out, HS, CS)
    dxs = torch.empty(n, 3 * C)
    G = torch.empty(2, 4 * H + 1, C + 2 * H + 1)
    K.jk_bwd_params(c.xs, c.dout, n, npad, C, c.lstm, c.w_att, c.b_att, HS, CS, dxs, G)
    return Bag(out=out, HS=HS[:, :n], CS=CS[:, :n], dxs=dxs, grads=unpack_G(G, C))


def chain_order(K, order):
    """Summation orders of a K-term dot product: 'ascending', or 'interleaved' = the k order of the matrix-core kernels (within each
    group of eight: 0, 4, 1, 5, 2, 6, 3, 7 -- v_mfma_f32_32x32x2_f32 takes one k from each lane half per instruction)."""
    if order == 'ascending':
        return list(range(K))
    assert order == 'interleaved'
    return [k for q in range((K + 7) // 8) for t in range(4) for k in (8 * q + t, 8 * q + 4 + t) if k < K]


@functools.lru_cache(maxsize=None)
def chain_forward(C, n, kind, order):
    """The forward with every gate pre-activation accumulated as ONE float32 FMA chain (bias, then the x terms, then the h terms, each
    in ``order``) and correctly rounded activations: what a float32 kernel computes at best, and a probe of an input's conditioning
    that does not depend on the summation order a BLAS happens to use.  Returns a Bag: out, HS, CS (float32 values)."""
    c = case(C, n, kind)
    H = c.H
    x = c.xs.numpy().reshape(n, 3, C)
    sig = lambda v: _f32(1.0 / (1.0 + np.exp(-np.clip(v.astype(np.float64), -700, 700))))
    tanh = lambda v: _f32(np.tanh(v.astype(np.float64)))
    HS, CS = np.zeros((6 * H, n), np.float32), np.zeros((6 * H, n), np.float32)
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = [p.numpy() for p in c.lstm[4 * d:4 * d + 4]]
        h, cell = np.zeros((n, H), np.float32), np.zeros((n, H), np.float32)
        for s in range(3):
            t = s if d == 0 else 2 - s
            pre = np.tile(b_ih + b_hh, (n, 1))
            for k in chain_order(C, order):
                pre = _fma(x[:, t, k:k + 1], w_ih[None, :, k], pre)
            for k in chain_order(H, order) if s > 0 else ():
                pre = _fma(h[:, k:k + 1], w_hh[None, :, k], pre)
            i, f, g, o = sig(pre[:, :H]), sig(pre[:, H:2 * H]), tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
            cell = f * cell + i * g
            h = o * tanh(cell)
            HS[(d * 3 + t) * H:(d * 3 + t + 1) * H], CS[(d * 3 + t) * H:(d * 3 + t + 1) * H] = h.T, cell.T
    HS, CS = torch.from_numpy(HS), torch.from_numpy(CS)
    hs = HS.double().reshape(2, 3, H, n)
    score = torch.stack([hs[0, t].t() @ c.w_att[:H].double() + hs[1, t].t() @ c.w_att[H:].double() for t in range(3)], 1)
    out = (c.xs.double().reshape(n, 3, C) * torch.softmax(score, 1).unsqueeze(-1)).sum(1)
    return Bag(out=out, HS=HS, CS=CS)


EDGE_C = (20, 4, 6, 30)
EDGE_N = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)
SATURATED_C = (4, 6, 20, 32)


def gpu_inputs():
    """Every (C, n, kind) a GPU test runs: the CPU tests hold the float32 twin to the yardstick on each of them."""
    cases = [(C, 77, 'plain') for C in ALL_C]
    cases += [(C, n, 'plain') for C in EDGE_C for n in EDGE_N]
    cases += [(C, 1025, 'plain') for C in MATRIX_CORE_C]
    cases += [(20, 2500, 'plain')]
    cases += [(C, 77, 'saturated') for C in SATURATED_C]
    return sorted(set(cases))


def excesses(got, ref):
    """{tensor name: elementwise_excess at the project's rtol = 1e-4}, one entry per tensor."""
    want = dict(tensors(ref))
    return {k: elementwise_excess(v, want[k]) for k, v in tensors(got)}


@functools.lru_cache(maxsize=None)
def twin_excess(C, n, kind='plain'):
    return excesses(case_twin(C, n, kind), case_reference(C, n, kind))


# ---------------------------------------------------------------------------------------------- activation readout
def readout_weights(C, gate):
    """LSTM parameters (float32) with which a kernel prints its own activation function: w_hh = 0; the w_ih rows of ``gate`` are
    one-hot (unit j reads input k = j mod C) and that gate's bias is 0; the gate it is multiplied with is driven to exactly 1 by
    a bias of 40 (gate 'g': i = sigmoid(40); gate 'i': g = tanh(40)).  At the first step of a direction the cell state is zero, so
    CS[d=0, t=0, j, node] = act(x[node, 0, j mod C]) and CS[d=1, t=2, j, node] = act(x[node, 2, j mod C]), products with 0 and 1 being exact."""
    H = 3 * C // 2
    row0 = {'i': 0, 'g': 2 * H}[gate]
    ones = {'i': 2 * H, 'g': 0}[gate]
    lstm = []
    for _ in range(2):
        w_ih = torch.zeros(4 * H, C)
        for j in range(H):
            w_ih[row0 + j, j % C] = 1.0
        b_ih = torch.zeros(4 * H)
        b_ih[ones:ones + H] = 40.0
        lstm += [w_ih, torch.zeros(4 * H, H), b_ih, torch.zeros(4 * H)]
    return lstm


def sweep():
    """tanh arguments (float32): 4096 magnitudes log-spaced in [1e-6, 20], both signs, and the branch point 1/4 of fast_tanh with its
    two float32 neighbours."""
    m = np.logspace(np.log10(1e-6), np.log10(20.0), 4096).astype(np.float32)
    q = np.float32(0.25)
    m = np.concatenate([m, [np.nextafter(q, np.float32(0)), q, np.nextafter(q, np.float32(1))]]).astype(np.float32)
    return np.concatenate([m, -m])


def sigmoid_sweep():
    """sigmoid arguments (float32): 8001 points in [-30, 30], and +-80, +-87, +-88, +-100 around the clamp of fast_sigmoid."""
    far = np.array([80, 87, 88, 100], dtype=np.float32)
    return np.concatenate([np.linspace(-30, 30, 8001).astype(np.float32), far, -far])


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def _fma(a, b, c):          # float32 fused multiply-add: the product of two float32 is exact in float64
    return _f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def _exp32(x, shift):
    """Correctly rounded float32 exp of a float32 argument, moved by ``shift`` float32 ulp (standing for __expf)."""
    e = _f32(np.exp(x.astype(np.float64)))
    for _ in range(abs(shift)):
        e = np.nextafter(e, np.float32(np.inf if shift > 0 else -np.inf))
    return e


def fast_tanh_model(x, shift=0):
    """fast_tanh of csrc/jk_mfma.hip in float32 numpy: |x| < 1/4: the odd Taylor polynomial to x^9 in Horner form with FMAs;
    else (1 - e) / (1 + e), e = exp(-2|x|), the reciprocal taken as correctly rounded (v_rcp_f32 + one Newton step)."""
    x = np.asarray(x, dtype=np.float32)
    one = np.float32(1)
    ax, x2 = np.abs(x), x * x
    e = _exp32(np.float32(-2) * ax, shift)
    big = (one - e) * _f32(1.0 / (one + e).astype(np.float64))
    c = [np.float32(62) / np.float32(2835), np.float32(-17) / np.float32(315), np.float32(2) / np.float32(15),
         np.float32(-1) / np.float32(3), one]
    p = np.full_like(x2, c[0])
    for ck in c[1:]:
        p = _fma(x2, p, np.full_like(x2, ck))
    small = ax * p
    return np.copysign(np.where(ax < np.float32(0.25), small, big), x).astype(np.float32)


def one_line_tanh_model(x, shift=0):
    """The rejected form 2 / (1 + exp(-2x)) - 1 in float32: about 2^-24 of ABSOLUTE error."""
    x = np.asarray(x, dtype=np.float32)
    one = np.float32(1)
    e = _exp32(np.float32(-2) * x, shift)
    return (_f32(2.0 / (one + e).astype(np.float64)) - one).astype(np.float32)


def rel_ulps(got, want64):
    """|got - want| / |want| in units of 2^-23, elementwise (0 where want is 0 and got is too)."""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.abs(got - want64) / np.abs(want64) / ULP
    return np.where(want64 == 0, np.where(got == 0, 0.0, np.inf), r)
