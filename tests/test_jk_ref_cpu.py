"""CPU: the float64 DenseJK reference of tests/jk_ref.py against torch.nn.LSTM, the float32 twin (oracle/flat_ref.TorchKernels)
against that reference on every input the GPU tests run, the activation-readout weights, the float32 models behind the readout
bound of tests/test_jk_gpu.py, and the npad refusals of the library (they launch nothing, so they run without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import _abi, kernels
import jk_ref as R
from util import elementwise_excess


@pytest.mark.parametrize('C,n', [(2, 5), (6, 33), (20, 40)])
def test_manual_loop_is_torch_nn_lstm(C, n):
    """Forward and every gradient of the manual loop agree with nn.LSTM(bidirectional) + Linear + softmax in float64 to 1e-12."""
    H = 3 * C // 2
    torch.manual_seed(C)
    mod = torch.nn.LSTM(C, H, bidirectional=True, batch_first=True).double()
    att = torch.nn.Linear(2 * H, 1).double()
    xs = torch.randn(n, 3 * C, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(n, C, dtype=torch.float64)
    names = ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')
    ps = [getattr(mod, k) for k in names] + [getattr(mod, k + '_reverse') for k in names]
    seq = xs.reshape(n, 3, C)
    alpha, _ = mod(seq)
    score = att(alpha).squeeze(-1)
    score.retain_grad()
    want = (seq * torch.softmax(score, dim=-1).unsqueeze(-1)).sum(1)
    want.backward(dout)
    ref = R.reference(xs, ps, att.weight, att.bias, dout)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(ref.out, want.detach()) and close(ref.score, score.detach()) and close(ref.ds, score.grad)
    assert close(ref.dxs, xs.grad)
    for g, p in zip(ref.grads, ps + [att.weight, att.bias]):
        assert g.shape == p.grad.shape and close(g, p.grad)
    # saved states: forward-direction hidden state of time t = alpha[:, t, :H], reverse = alpha[:, t, H:]
    for d in range(2):
        for t in range(3):
            assert close(ref.HS[(d * 3 + t) * H:(d * 3 + t + 1) * H].t(), alpha[:, t, d * H:(d + 1) * H].detach())
    # the layout of G that the kernels and unpack_G share, against kernels.split_jk_param_grads
    flat = torch.cat([g.reshape(-1) for g in ref.grads])
    for g, v in zip(ref.grads, kernels.split_jk_param_grads(flat, C)):
        assert torch.equal(g, v)


def test_twin_is_conditioned_on_every_gpu_input():
    """The float32 twin meets the elementwise yardstick with room on every input of tests/test_jk_gpu.py: at most 0.25 for every
    tensor of a plain input and for the forward tensors of a saturated one (whose gradients are judged against 4 x the twin's
    own excess), and a quarter of the bound for d att.bias.  An input that breaks this is a bad input: change it, not the bound."""
    worst = {}
    for C, n, kind in R.gpu_inputs():
        ref = R.case_reference(C, n, kind)
        for k, e in R.twin_excess(C, n, kind).items():
            assert np.isfinite(e)
            if kind == 'plain' or k in ('out', 'HS', 'CS'):
                assert e <= 0.25, (C, n, kind, k, e)
            worst[(kind, k)] = max(worst.get((kind, k), 0.0), e)
        assert abs(float(R.case_twin(C, n, kind).grads[9])) <= 0.25 * R.db_att_bound(ref), (C, n, kind)
    print({'%s %s' % k: round(v, 3) for k, v in sorted(worst.items())})


@pytest.mark.parametrize('C', R.SATURATED_C)
def test_saturated_inputs_are_conditioned_under_every_summation_order(C):
    """With pre-activations in the thousands, the twin's 0.25 says little: it is ONE float32 summation order (the BLAS's).  The
    forward as a single float32 FMA chain, ascending (the thread-per-direction kernels) and in the matrix-core kernels' interleaved
    k order, with correctly rounded activations, stays within 0.25 as well -- so the forward bound of 1 asks nothing of a kernel
    but float32 arithmetic and accurate activations."""
    ref = R.case_reference(C, 77, 'saturated')
    for order in ('ascending', 'interleaved'):
        ch = R.chain_forward(C, 77, 'saturated', order)
        for k in ('out', 'HS', 'CS'):
            e = elementwise_excess(getattr(ch, k), getattr(ref, k))
            assert e <= 0.25, (C, order, k, e)
    assert R.chain_order(12, 'interleaved') == [0, 4, 1, 5, 2, 6, 3, 7, 8, 9, 10, 11]
    assert sorted(R.chain_order(30, 'interleaved')) == list(range(30))


def test_inputs_cover_the_edges():
    c = R.case(20, 77)
    assert not c.xs[3].any() and float(c.xs[8:16].abs().max()) < 0.01 and float(c.xs[16:24].abs().max()) > 30
    s = R.case(20, 77, 'saturated')                        # (a draw of its own: jk_ref.SATURATED_DRAW)
    assert not s.xs[3].any() and float(s.xs[8:16].abs().max()) < 0.1 and float(s.xs[16:24].abs().max()) > 300
    assert float(s.lstm[0].abs().max()) > 4 / 30 ** 0.5 and float(s.w_att.abs().max()) <= 1 / 60 ** 0.5
    ref = R.case_reference(20, 77, 'saturated')            # gates really saturate: a tenth of the cell states sit at |c| > 0.999
    assert float((ref.CS.abs() > 0.999).double().mean()) > 0.1


@pytest.mark.parametrize('gate', ['g', 'i'])
@pytest.mark.parametrize('C', [4, 6, 20])
def test_readout_weights_print_the_activation(C, gate):
    H = 3 * C // 2
    pts = torch.from_numpy(R.sweep() if gate == 'g' else R.sigmoid_sweep()).double()
    xs = pts.reshape(-1, 1).repeat(1, 3 * C)
    lstm = [p.double() for p in R.readout_weights(C, gate)]
    _, _, CS, _ = R.forward(xs, lstm, torch.zeros(2 * H, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
    want = torch.tanh(pts) if gate == 'g' else torch.sigmoid(pts)
    assert torch.sigmoid(torch.tensor(40.0)).item() == 1.0 and torch.tanh(torch.tensor(40.0)).item() == 1.0      # in float32
    for rows in (CS[0:H], CS[5 * H:6 * H]):                 # d = 0 at t = 0, d = 1 at t = 2: first step of a direction
        assert float((rows - want.unsqueeze(0)).abs().max()) <= 1e-15


def test_fast_tanh_model_and_the_readout_bound():
    """Where the readout bound of 8 x 2^-23 comes from: the stated fast_tanh algorithm with a correctly rounded exp has at most
    2 units of relative error over the sweep (numpy's float32 tanh: about 1); an exp that is 2 ulp off (__expf) brings it to
    between 4 and 5, so the bound leaves a factor of about 2; the rejected one-line form exceeds the bound by far more than a
    factor of 2 wherever |x| <= 0.1 matters, so the GPU readout catches that regression."""
    x = R.sweep()
    assert x.dtype == np.float32 and x.size == 2 * (4096 + 3) and np.float32(0.25) in x
    assert np.abs(x).min() == np.float32(1e-6) and np.abs(x).max() == np.float32(20.0)
    want = np.tanh(x.astype(np.float64))
    e0 = R.rel_ulps(R.fast_tanh_model(x), want).max()
    e2 = max(R.rel_ulps(R.fast_tanh_model(x, s), want).max() for s in (2, -2))
    enp = R.rel_ulps(np.tanh(x), want).max()
    small = np.abs(x) <= 0.1
    one = [R.rel_ulps(R.one_line_tanh_model(x, s), want) for s in (0, 2, -2)]
    print('fast_tanh model %.2f, exp +-2 ulp %.2f, numpy float32 %.2f; one-line form: %.3g at |x| <= 0.1, %.3g near 1e-6' % (
        e0, e2, enp, min(o[small].max() for o in one), min(o[np.abs(x) < 2e-6].max() for o in one)))
    assert e0 <= 2.0 and enp <= 2.0
    assert 2.0 < e2 <= 5.0 and 1.5 * e2 <= R.READOUT_ULPS
    for o in one:
        assert o[small].max() >= 2 * R.READOUT_ULPS
        assert o[np.abs(x) < 2e-6].max() > 1e5
        # ... and not through a single unlucky point: a third of the sweep below 0.1 breaks the bound
        assert (o[small] > R.READOUT_ULPS).mean() > 1 / 3


def test_sigmoid_sweep():
    s = R.sigmoid_sweep()
    assert s.dtype == np.float32 and s.size == 8001 + 8 and s.min() == -100 and s.max() == 100
    assert {80.0, 87.0, 88.0, -80.0, -87.0, -88.0} <= set(s.tolist())


# ---------------------------------------------------------------------------------------------- the npad contract
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(kernels.lib_path())
    _abi.declare(lib)
    return lib


@pytest.mark.parametrize('n,npad', [(37, 37), (37, 32), (65, 64), (1, 0), (33, 96), (100, 1000), (5, -64)])
@pytest.mark.parametrize('C', [4, 6, 20, 30])
def test_every_entry_point_refuses_a_bad_npad_before_it_touches_anything(lib, C, n, npad):
    """npad >= n and npad % 64 == 0 (include/cgc_hip.h), checked in front of everything else: with NULL for every pointer the four
    entry points return CGC_EINVAL -- no argument was read, nothing was launched (this host has no GPU to launch on)."""
    assert npad < n or npad % 64 != 0
    N = None
    assert lib.cgc_jk_lstm_fwd(N, n, npad, C, N, N, N, N, N, N, N) == -1
    assert lib.cgc_jk_lstm_bwd(N, N, n, npad, C, N, N, N, N, N, N, N, N, N, N) == -1
    assert lib.cgc_jk_lstm_bwd_params(N, N, n, npad, C, N, N, N, N, N, N, N, N, N) == -1
    assert lib.cgc_jk_lstm_bwd_flat(N, N, n, npad, C, N, N, N, N, N, N, N, N, N) == -1


def test_no_rows_is_not_an_error(lib):
    N = None
    assert lib.cgc_jk_lstm_fwd(N, 0, 37, 20, N, N, N, N, N, N, N) == 0
    assert lib.cgc_jk_lstm_bwd_flat(N, N, 0, 0, 20, N, N, N, N, N, N, N, N, N) == 0

