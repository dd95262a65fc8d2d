"""GPU: the DenseJK kernels (csrc/jk.hip, csrc/jk_mfma.hip) against the float64 reference of tests/jk_ref.py, tensor by tensor and
element by element: every compiled channel count, the row counts around the 32-node tiles, the unaligned fallback, the entry point the
step sequencer calls (cgc_jk_lstm_bwd_flat), determinism, saturated gates, the npad contract -- and a readout of the kernels' own
tanh / sigmoid.

Yardstick: util.elementwise_excess(got, ref64) at rtol = 1e-4 for out, HS[:, :n], CS[:, :n], dxs and each parameter gradient apart,
bounded by max(1, 4 * e32) with e32 the excess of the float32 torch twin on the same input (tests/test_jk_ref_cpu.py holds e32 to
0.25 on the plain inputs, so the bound is 1 there).  d att.bias, mathematically zero, is held to 1e-4 * sum |ds|.  Every buffer a
kernel writes or uses as scratch is filled with NaN first, padding columns of HS / CS included, and ``out`` / ``dxs`` are the first n
rows of larger allocations whose other elements must keep their 7.0."""
import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels
import jk_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def up(n, m=1024):
    return -(-n // m) * m


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


class Guarded(object):
    """A [rows, cols] float32 view inside a larger allocation filled with 7.0; ``unaligned``: the view starts one float past a
    16-byte boundary (torch's allocations start 256-byte aligned)."""

    def __init__(self, rows, cols, unaligned=False, data=None):
        self.off, self.numel = (1 if unaligned else 0), rows * cols
        self.buf = torch.full((self.numel + 4 * cols + 8,), 7.0, dtype=torch.float32, device=DEV)
        self.v = self.buf[self.off:self.off + self.numel].view(rows, cols)
        assert self.v.data_ptr() % 16 == (4 if unaligned else 0)
        if data is None:
            self.v.fill_(NAN)
        else:
            self.v.copy_(data)

    def intact(self):
        return bool((self.buf[:self.off] == 7.0).all()) and bool((self.buf[self.off + self.numel:] == 7.0).all())


class Io(object):
    """Device buffers of one input, as the production caller has them (torch.empty, here: NaN) plus guard rows."""

    def __init__(self, c, npad, unaligned=False):
        C, H, n = c.C, c.H, c.n
        self.c, self.npad = c, npad
        self.xs, self.dout = Guarded(n, 3 * C, unaligned, c.xs), Guarded(n, C, unaligned, c.dout)
        self.out, self.dxs = Guarded(n, C, unaligned), Guarded(n, 3 * C, unaligned)
        self.lstm = [p.to(DEV) for p in c.lstm]
        self.w_att, self.b_att = c.w_att.to(DEV), c.b_att.to(DEV)
        self.HS, self.CS = nans(6 * H, npad), nans(6 * H, npad)

    def fwd(self):
        c = self.c
        hip().jk_fwd(self.xs.v, c.n, self.npad, c.C, self.lstm, self.w_att, self.b_att, self.out.v, self.HS, self.CS)
        assert self.out.intact() and self.xs.intact()
        for t in (self.out.v, self.HS[:, :c.n], self.CS[:, :c.n]):
            assert bool(torch.isfinite(t).all())

    def staged(self):
        """jk_bwd -> (dxs, the ten gradients out of DGT_d @ INT_d^T over all 3 * npad columns, in float64)."""
        c, npad = self.c, self.npad
        C, H, n = c.C, c.H, c.n
        DGT, INT, DHC = nans(2, 4 * H + 1, 3 * npad), nans(2, C + 2 * H + 1, 3 * npad), nans(2, 2, H, npad)
        self.dxs.v.fill_(NAN)
        hip().jk_bwd(self.xs.v, self.dout.v, n, npad, C, self.lstm, self.w_att, self.b_att, self.HS, self.CS, self.dxs.v, DGT, INT, DHC)
        assert self.dxs.intact() and bool(torch.isfinite(self.dxs.v).all())
        assert bool(torch.isfinite(DGT).all()) and bool(torch.isfinite(INT).all())       # every column is written ...
        for T in (DGT.view(2, 4 * H + 1, 3, npad), INT.view(2, C + 2 * H + 1, 3, npad)):
            assert not bool(T[..., n:].any())                                            # ... padding drops out of the product
        G = torch.stack([DGT[d].double().cpu() @ INT[d].double().cpu().t() for d in range(2)])
        return self.dxs.v.cpu().clone(), R.unpack_G(G, C)

    def params(self):
        """jk_bwd_params + jk_unpack_param_grads -> (dxs, the ten gradients, G)."""
        c = self.c
        C, H, n = c.C, c.H, c.n
        G = nans(2, 4 * H + 1, C + 2 * H + 1)
        self.dxs.v.fill_(NAN)
        hip().jk_bwd_params(self.xs.v, self.dout.v, n, self.npad, C, self.lstm, self.w_att, self.b_att, self.HS, self.CS, self.dxs.v, G)
        assert self.dxs.intact() and bool(torch.isfinite(self.dxs.v).all())
        assert bool(torch.isfinite(G).all())              # rows and columns outside the documented blocks: written, never used
        grads = [g.cpu().clone() for g in hip().jk_unpack_param_grads(G, C)]
        for a, b in zip(grads, R.unpack_G(G.cpu(), C)):
            assert torch.equal(a.reshape(-1), b.reshape(-1))
        return self.dxs.v.cpu().clone(), grads, G

    def raw(self, entry, target, ws):
        """lib.cgc_jk_lstm_bwd_params / cgc_jk_lstm_bwd_flat called directly: the return code."""
        c, K = self.c, hip()
        p = kernels._ptr
        arr = K._ptr_array(self.lstm)
        return getattr(K.lib, entry)(p(self.xs.v), p(self.dout.v), c.n, self.npad, c.C, arr, p(self.w_att), p(self.b_att), p(self.HS),
                                     p(self.CS), p(self.dxs.v), p(target), p(ws), K._stream())

    def got(self, dxs, grads):
        n = self.c.n
        return R.Bag(out=self.out.v.cpu(), HS=self.HS[:, :n].cpu(), CS=self.CS[:, :n].cpu(), dxs=dxs, grads=grads)


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))        # (NaN fills compare equal)


def workspace(C):
    return nans(int(hip().lib.cgc_jk_bwd_ws_floats(C)))


def judge(got, C, n, kind, what):
    """Print every figure, then hold each tensor to max(1, 4 * twin excess) and d att.bias to 1e-4 * sum |ds|."""
    ref, e32 = R.case_reference(C, n, kind), R.twin_excess(C, n, kind)
    ex = R.excesses(got, ref)
    db, db_bound = abs(float(got.grads[9])), R.db_att_bound(ref)
    print('JK %s C=%d n=%d %s: ' % (what, C, n, kind) + ' '.join('%s=%.3f(%.3f)' % (k, ex[k], e32[k]) for k in ex)
          + ' db_att=%.3g(bound %.3g)' % (db, db_bound))
    bad = {k: (e, max(1.0, 4 * e32[k])) for k, e in ex.items() if not e <= max(1.0, 4 * e32[k])}
    assert not bad, (what, C, n, kind, bad)
    assert db <= db_bound, (what, C, n, kind, db, db_bound)


def full_check(C, n, npad, kind='plain', unaligned=False, staged=True):
    io = Io(R.case(C, n, kind), npad, unaligned)
    io.fwd()
    if staged:
        judge(io.got(*io.staged()), C, n, kind, 'jk_bwd npad=%d' % npad)
    dxs, grads, G = io.params()
    judge(io.got(dxs, grads), C, n, kind, 'jk_bwd_params npad=%d%s' % (npad, ' unaligned' if unaligned else ''))
    return io, G


# ---------------------------------------------------------------------------------------------- 1: every compiled channel count
@pytest.mark.parametrize('C', R.ALL_C)
def test_every_channel_count(C):
    """n = 77 = two full 32-node tiles and a tail of 13.  C = 2, 10, 14, 18, 22, 26, 28, 30 ran in no test before this one
    (26-30: over 64 KB of LDS); 4, 8, 12, 16, 20 run on the matrix cores, but for jk_bwd, which is k_jk_bwd<C> for every C
    (there on HS / CS of the matrix-core forward)."""
    K = hip()
    assert K.jk_supported(C) and bool(K.lib.cgc_jk_matrix_core(C)) == (C in R.MATRIX_CORE_C)
    H = 3 * C // 2
    io, G = full_check(C, 77, 1024)
    if C in R.MATRIX_CORE_C:        # in-kernel parameter gradients: what is no gradient is zero (include/cgc_hip.h)
        G = G.cpu()
        assert not G[:, :4 * H, C + H + 1:].any() and not G[:, 4 * H, :C + H].any() and not G[1, 4 * H, C + H].any()


def test_unsupported_channel_counts_are_refused():
    K = hip()
    for C in (0, 1, 3, 7, 21, 34):
        assert not K.jk_supported(C) and not K.lib.cgc_jk_matrix_core(C)


# ---------------------------------------------------------------------------------------------- 2: row-count edges
@pytest.mark.parametrize('n', R.EDGE_N)
@pytest.mark.parametrize('C', R.EDGE_C)
def test_row_count_edges(C, n):
    full_check(C, n, up(n))


@pytest.mark.parametrize('C', R.EDGE_C)
def test_padding_wider_than_a_tile_pair(C):
    full_check(C, 33, 2048)


# ---------------------------------------------------------------------------------------------- 3: unaligned fallback
@pytest.mark.parametrize('C', [4, 12, 20])
def test_unaligned_fallback(C):
    """xs, out, dout, dxs one float past a 16-byte boundary: the matrix-core kernels refuse, k_jk_fwd<C> / k_jk_bwd<C> and the
    sliced GEMMs of HipKernels.jk_bwd_params take over."""
    io, _ = full_check(C, 77, 1024, unaligned=True, staged=False)
    H = 3 * C // 2
    G, ws = nans(2, 4 * H + 1, C + 2 * H + 1), workspace(C)
    before = io.dxs.buf.clone()
    assert io.raw('cgc_jk_lstm_bwd_params', G, ws) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(G).all()) and bool(torch.isnan(ws).all()) and bits_equal(io.dxs.buf, before)     # nothing launched


@pytest.mark.parametrize('C', [4, 20, 6])
def test_staged_backward_ignores_alignment(C):
    """jk_bwd on the same HS / CS / weights, once with aligned xs / dout / dxs and once with copies one float past a 16-byte
    boundary: one kernel (k_jk_bwd<C>) for both, so dxs, DGT and INT agree bit for bit, padded columns included."""
    n, npad, H = 77, 1024, 3 * C // 2
    io = Io(R.case(C, n), npad)
    io.fwd()
    got = []
    for unaligned in (False, True):
        xs, dout = Guarded(n, 3 * C, unaligned, io.xs.v), Guarded(n, C, unaligned, io.dout.v)
        dxs = Guarded(n, 3 * C, unaligned)
        DGT, INT, DHC = nans(2, 4 * H + 1, 3 * npad), nans(2, C + 2 * H + 1, 3 * npad), nans(2, 2, H, npad)
        hip().jk_bwd(xs.v, dout.v, n, npad, C, io.lstm, io.w_att, io.b_att, io.HS, io.CS, dxs.v, DGT, INT, DHC)
        assert dxs.intact() and xs.intact() and dout.intact()
        got.append((dxs.v.contiguous(), DGT, INT))
    for name, a, b in zip(('dxs', 'DGT', 'INT'), got[0], got[1]):
        assert bits_equal(a, b), name


# ---------------------------------------------------------------------------------------------- 4: cgc_jk_lstm_bwd_flat
@pytest.mark.parametrize('n', [77, 1025])
@pytest.mark.parametrize('C', R.MATRIX_CORE_C)
def test_bwd_flat(C, n):
    """The entry the step sequencer calls, with a NaN-filled workspace of cgc_jk_bwd_ws_floats(C)."""
    io = Io(R.case(C, n), up(n))
    io.fwd()
    flat, ws = nans(int(hip().lib.cgc_jk_param_grad_floats(C))), workspace(C)
    assert io.raw('cgc_jk_lstm_bwd_flat', flat, ws) == 0
    assert io.dxs.intact() and bool(torch.isfinite(io.dxs.v).all()) and bool(torch.isfinite(flat).all())
    dxs = io.dxs.v.cpu().clone()
    grads = [g.cpu() for g in kernels.split_jk_param_grads(flat, C)]
    judge(io.got(dxs, grads), C, n, 'plain', 'jk_bwd_flat')
    dxs2, grads2, _ = io.params()
    same = torch.equal(dxs, dxs2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    print('JK jk_bwd_flat C=%d n=%d bit-equal to jk_bwd_params + unpack: %s' % (C, n, same))


def test_bwd_flat_refuses_what_it_cannot_run():
    for C, unaligned in ((6, False), (20, True)):
        io = Io(R.case(C, 77), 1024, unaligned)
        io.fwd()
        flat, ws = nans(int(hip().lib.cgc_jk_param_grad_floats(C))), workspace(C)
        before = io.dxs.buf.clone()
        assert io.raw('cgc_jk_lstm_bwd_flat', flat, ws) == -1
        torch.cuda.synchronize()
        assert bool(torch.isnan(flat).all()) and bool(torch.isnan(ws).all()) and bits_equal(io.dxs.buf, before)


# ---------------------------------------------------------------------------------------------- 5: determinism
def test_bwd_params_is_deterministic():
    """More tiles (79) than one fold of 16 partials: both reduction stages add in a fixed order."""
    C, n = 20, 2500
    io = Io(R.case(C, n), up(n))
    io.fwd()
    dxs1, grads1, G1 = io.params()
    dxs2, grads2, G2 = io.params()
    assert torch.equal(dxs1, dxs2) and torch.equal(G1, G2)
    judge(io.got(dxs1, grads1), C, n, 'plain', 'jk_bwd_params')


# ---------------------------------------------------------------------------------------------- 6: activation readout
def _readout(C, gate, unaligned):
    """CS of the first step of each direction under readout_weights: the kernel's own tanh / sigmoid of every sweep point, [2, H, n]."""
    pts = R.sweep() if gate == 'g' else R.sigmoid_sweep()
    n, H = pts.size, 3 * C // 2
    xs = torch.from_numpy(pts).reshape(n, 1).repeat(1, 3 * C)
    gen = torch.Generator().manual_seed(C)
    c = R.Bag(C=C, H=H, n=n, xs=xs, dout=torch.zeros(n, C), lstm=R.readout_weights(C, gate),
              w_att=torch.rand(2 * H, generator=gen) - 0.5, b_att=torch.zeros(1))
    io = Io(c, up(n), unaligned)
    io.fwd()
    CS = io.CS[:, :n].cpu().double().numpy()
    return pts, np.stack([CS[0:H], CS[5 * H:6 * H]])


READOUT = [(4, False, 'matrix-core'), (20, False, 'matrix-core'), (6, False, 'thread-per-direction'), (4, True, 'k_jk_fwd<4> (unaligned)')]


@pytest.mark.parametrize('C,unaligned,family', READOUT)
def test_tanh_readout(C, unaligned, family):
    """The kernel's tanh against float64 tanh over jk_ref.sweep(): at most 8 x 2^-23 relative (derivation: test_jk_ref_cpu.py).
    Measured on an MI355X: see DESIGN.md, DenseJK."""
    pts, got = _readout(C, 'g', unaligned)
    err = R.rel_ulps(got, np.tanh(pts.astype(np.float64))[None, None, :])
    a = np.abs(pts)
    print('JK tanh readout C=%d %s: max %.2f x 2^-23 (|x| < 1/4: %.2f, >= 1/4: %.2f)' % (
        C, family, err.max(), err[..., a < 0.25].max(), err[..., a >= 0.25].max()))
    assert np.isfinite(got).all() and err.max() <= R.READOUT_ULPS


@pytest.mark.parametrize('C,unaligned,family', READOUT)
def test_sigmoid_readout(C, unaligned, family):
    """The kernel's sigmoid against float64: 8 x 2^-23 relative on [-80, 30]; below -80 (the fminf(-x, 87) clamp) at most 1e-37
    absolute, above 30 at most 2^-24 below 1; finite everywhere."""
    pts, got = _readout(C, 'i', unaligned)
    x = pts.astype(np.float64)
    want = 1.0 / (1.0 + np.exp(-x))
    mid, lo, hi = (pts >= -80) & (pts <= 30), pts < -80, pts > 30
    err = R.rel_ulps(got[..., mid], want[None, None, mid])
    worst = np.unravel_index(np.argmax(err), err.shape)[-1]
    print('JK sigmoid readout C=%d %s: max %.2f x 2^-23 at x = %g (x >= -10: %.2f); below -80: abs %.3g; above 30: 1 - s <= %.3g' % (
        C, family, err.max(), pts[mid][worst], err[..., pts[mid] >= -10].max(), np.abs(got[..., lo] - want[None, None, lo]).max(),
        (1.0 - got[..., hi]).max()))
    assert np.isfinite(got).all()
    assert np.abs(got[..., lo] - want[None, None, lo]).max() <= 1e-37
    assert (got[..., hi] <= 1.0).all() and (1.0 - got[..., hi]).max() <= 2.0 ** -24
    assert err.max() <= R.READOUT_ULPS


# ---------------------------------------------------------------------------------------------- 7: saturated gates
@pytest.mark.parametrize('C', R.SATURATED_C)
def test_saturated_gates(C):
    """LSTM weights x 8, xs x 10 (the x 30 rows reach pre-activations of several thousand), attention unscaled: everything finite,
    forward tensors within the plain yardstick, gradients within 4 x the twin's own excess (about 2 for dxs at C = 32: a fixed
    number would be wrong).  The input is conditioned under every float32 summation order (test_jk_ref_cpu.py), not only the
    twin's: on the plain draw scaled, the matrix-core forward at C = 20 measured 2.73 for HS in ONE element, and a float32 FMA
    chain in its k order, on the CPU, gives the same 2.73 -- the input's doing (jk_ref.SATURATED_DRAW), not the kernel's."""
    full_check(C, 77, 1024, kind='saturated')


# ---------------------------------------------------------------------------------------------- the npad contract on the device
@pytest.mark.parametrize('C', [20, 6])
def test_refused_npad_touches_nothing(C):
    """npad = n = 37 (no multiple of 64): all four entry points refuse and every buffer keeps its fill."""
    K = hip()
    io = Io(R.case(C, 37), 37)
    H = 3 * C // 2
    with pytest.raises(RuntimeError, match='cgc_jk_lstm_fwd failed with code -1'):
        K.jk_fwd(io.xs.v, 37, 37, C, io.lstm, io.w_att, io.b_att, io.out.v, io.HS, io.CS)
    DGT, INT, DHC = nans(2, 4 * H + 1, 3 * 37), nans(2, C + 2 * H + 1, 3 * 37), nans(2, 2, H, 37)
    with pytest.raises(RuntimeError, match='cgc_jk_lstm_bwd failed with code -1'):
        K.jk_bwd(io.xs.v, io.dout.v, 37, 37, C, io.lstm, io.w_att, io.b_att, io.HS, io.CS, io.dxs.v, DGT, INT, DHC)
    G, flat, ws = nans(2, 4 * H + 1, C + 2 * H + 1), nans(int(K.lib.cgc_jk_param_grad_floats(C))), workspace(C)
    with pytest.raises(ValueError, match='multiple of 64'):
        K.jk_bwd_params(io.xs.v, io.dout.v, 37, 37, C, io.lstm, io.w_att, io.b_att, io.HS, io.CS, io.dxs.v, G)
    assert io.raw('cgc_jk_lstm_bwd_params', G, ws) == -1 and io.raw('cgc_jk_lstm_bwd_flat', flat, ws) == -1
    torch.cuda.synchronize()
    for t in (io.out.v, io.dxs.v, io.HS, io.CS, DGT, INT, DHC, G, flat, ws):
        assert bool(torch.isnan(t).all())


def test_staged_route_refuses_slices_that_do_not_divide():
    """C = 6 stages its parameter gradients through K slices of 768 columns: npad = 64 is fine for the library, not for them."""
    K = hip()
    C, n, npad = 6, 33, 64
    io = Io(R.case(C, n), npad)
    G = nans(2, 4 * 9 + 1, C + 2 * 9 + 1)
    with pytest.raises(ValueError, match='npad % 256 == 0'):
        K.jk_bwd_params(io.xs.v, io.dout.v, n, npad, C, io.lstm, io.w_att, io.b_att, io.HS, io.CS, io.dxs.v, G)
    torch.cuda.synchronize()
    assert bool(torch.isnan(G).all()) and bool(torch.isnan(io.dxs.v).all())
