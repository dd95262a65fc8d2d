"""GPU: the four kernels of csrc/head.hip (k_head_fwd, k_head_fwd_simple, k_head_bwd, k_head_bwd_simple) through the direct entry
points cgc_head_fwd / cgc_head_bwd against the float64 reference of tests/head_ref.py, element by element, on both sides of every
dispatch condition (tests/test_head_ref_cpu.py asserts that the cases lie where the table says and that every argument form meets
every kernel).

Yardsticks (tests/rowops_ref.py, tests/head_ref.py): keep exact; h exactly 0 where keep is 0; everything else |a-b| <= 1e-4 * terms +
1e-7 with terms the expression evaluated on magnitudes; exactly zero where the reference is exactly zero (a dropped unit at B = 1, a
gradient nobody asked for, softmax - onehot at L = 1); NaN exactly where the reference is NaN (all labels -100: the loss; a corrupt
label: the loss and every gradient).  An excess is the largest ratio of an error to its allowance; each is bounded by max(1, 4 * e32)
with e32 from the table E32 of tests/test_head_ref_cpu.py (empty: every bound is 1) and printed.

Per case and form: forward, then backward over the forward's own workspace (a batch of 128..164 graphs runs the simple forward and the
LDS backward over one workspace); every output sits in a canary-filled buffer of exactly the documented size (ws 3*B*H1 + B, logits
B*L, loss 1, scratch B*L + B*H1, grads H1*K + H1 + L*H1 + L, dx B*D each), aligned and one float past a 16-byte boundary; the loss
and per-sample slots keep the canary when y is NULL; a second launch on fresh buffers repeats every bit.  Beside that: the dropout
plane against head_ref.keep_plane bit for bit for seeds 0, 1, 2^63 and 2^64 - 1, equal bits of shared rows across the two routes of
either direction, corrupt labels, refusals, the autograd wrapper native._Head / native.head, and the model past both boundaries.

Which kernel ran where ((nseg, B, D, H1, L); every case runs head_ref.ROTATION, the first the full cross of head_ref.base_forms):
    k_head_fwd           (3,37,60,50,3) (3,127,60,50,3) (3,1,64,196,5) (1,4,8,6,8) (2,33,7,13,4) (1,1,1,1,1)
    k_head_fwd_simple    (3,128,60,50,3) (3,164,60,50,3) (3,165,60,50,3) (3,1,64,197,5) (3,40,300,50,3) (3,41,300,50,3) (1,4,8,6,9)
    k_head_bwd           every case but the two below
    k_head_bwd_simple    (3,165,60,50,3) (3,41,300,50,3)

Measured on an MI355X, largest excess per family over all cases, forms and both placements (the float32 twin on the CPU: 0.025):
    z / h                 0.0025  (3,164,60,50,3); keep exact everywhere
    logits and loss       0.00065 logits, 0.00053 per-sample loss, 0.00024 loss, all at (1,4,8,6,9)
    parameter gradients   0.0069  dW1 at (3,1,64,196,5); db1 0.0064, db2 0.0057, dW2 0.0029
    dx (and dl, dz)       0.0068  dx at (3,37,60,50,3); the scratch of k_head_bwd_simple: dl 0.058, dz 0.033 at (3,41,300,50,3)
    native.head (no biases, leaky ReLU, one readout): 0.0007 or less; the model at 130 and 170 graphs: logits, loss and the
    pred_model gradients within 3.5e-7 of the module stack (max-norm relative; bars 2e-6 and 5e-6)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import cgc_net_amd  # noqa: F401
from cgc_net_amd import kernels, native
from cgc_net_amd.data import Batch, SyntheticCellGraphs
import head_ref as H
from test_head_ref_cpu import bound

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OTHER_CASES = [c for c in H.CASES if c != H.BASE]


def hip():
    k = kernels.get()
    assert kernels.is_native()
    return k


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def launch(k, a, variant='aligned', backward=True):
    """Forward (and backward over its workspace) into fresh canary-guarded buffers -> (Place, outputs)."""
    P = H.Place(DEV, variant)
    o = H.run_forward(k, P, a)
    assert o['rc'] == 0, 'cgc_head_fwd refused %r' % (a.case,)
    if backward:
        b = H.run_backward(k, P, a, o)
        assert b['rc'] == 0, 'cgc_head_bwd refused %r' % (a.case,)
        o.update(b)
    return P, o


def twice(k, a, variant):
    """Two launches on fresh buffers: containment both times, identical bits."""
    (P1, o1), (P2, o2) = launch(k, a, variant), launch(k, a, variant)
    torch.cuda.synchronize()
    P1.check(), P2.check()
    for key in ('ws', 'logits', 'loss', 'scratch', 'grads'):
        assert same_bits(o1[key], o2[key]), 'second launch differs: ' + key
    for s in range(a.nseg):
        assert same_bits(o1['dx'][s], o2['dx'][s]), 'second launch differs: dx[%d]' % s
    return o1


def run_forms(case, forms, variant):
    k = hip()
    ex = H.Excess()
    for form in forms:
        a = H.arguments(case, form)
        ref = H.reference_of(case, form)
        o = twice(k, a, variant)
        one = H.Excess()
        H.judge_forward(a, ref, o, one)
        H.judge_backward(a, ref, o, one)
        bad = {n: e for n, e in one.items() if not e <= bound(case, n)}
        assert not bad, '%r %r %s: excess above its bound: %r' % (case, form, variant, bad)
        for n, e in one.items():
            ex.add(n, e)
    fam = ' '.join('%s=%.3g' % (f.replace(' ', '_'), max([ex[n] for n in names if n in ex] or [0.0])) for f, names in H.FAMILIES.items())
    print('HEAD %r %s fwd/bwd=%s/%s: %s | %s' % ((case, variant) + H.route(*case) + (ex.line(), fam)))


@pytest.mark.parametrize('act', H.ACTS)
def test_base_case_full_cross(act):
    """(3, 37, 60, 50, 3): activations x biases {both, none} x labels {valid, two -100, all -100, NULL} x gradients {dloss, dlogits_ext,
    both, neither} x p {0, 0.2, 0.5}, and the large logits."""
    run_forms(H.BASE, H.base_forms(act), 'aligned')


def test_base_case_misaligned():
    run_forms(H.BASE, H.ROTATION, 'misaligned')


@pytest.mark.parametrize('variant', ['aligned', 'misaligned'])
@pytest.mark.parametrize('case', OTHER_CASES)
def test_case(case, variant):
    run_forms(case, H.case_forms(case), variant)


# ---------------------------------------------------------------------------------------------- the dropout plane
def _prefix(a, B):
    """The first B samples of a call's operands, as a call of its own."""
    case = (a.nseg, B, a.D, a.H1, a.L)
    return H.Bag(case=case, form=a.form, seed=a.seed, nseg=a.nseg, B=B, D=a.D, H1=a.H1, L=a.L, K=a.K, xs=[x[:B].contiguous() for x in a.xs],
                 W1=a.W1, W2=a.W2, b1=a.b1, b2=a.b2, y=None if a.y is None else a.y[:B].contiguous(), act=a.act, p=a.p,
                 keep=a.keep[:B].contiguous(), dloss=a.dloss, ext=None if a.ext is None else a.ext[:B].contiguous())


@pytest.mark.parametrize('p', [0.2, 0.5])
@pytest.mark.parametrize('seed', H.SEEDS)
def test_keep_plane_is_the_stated_generator(seed, p):
    """Bit for bit, on the LDS route (B = 127) and on the simple route (B = 128): one plane on their shared rows."""
    k = hip()
    form = H.Form(1, True, 'valid', 'both', p, 'normal')
    planes = {}
    for B in (127, 128):
        a = H.arguments((3, B, 60, 50, 3), form, seed=seed)
        P, o = launch(k, a, backward=False)
        torch.cuda.synchronize()
        P.check()
        planes[B] = o['keep'].cpu()
        assert same_bits(planes[B], H.keep_plane(seed, B, 50, p)), (seed, p, B)
    assert H.route(3, 127, 60, 50, 3)[0] == 'lds' and H.route(3, 128, 60, 50, 3)[0] == 'simple'
    assert same_bits(planes[127], planes[128][:127])


# ---------------------------------------------------------------------------------------------- batch independence across routes
def test_forward_rows_do_not_depend_on_the_route():
    """Rows 0..126 of z, keep, h and logits from B = 127 (k_head_fwd) and from B = 128 (k_head_fwd_simple) on the same inputs: both
    are one fmaf chain in one order, so the bits are equal."""
    k = hip()
    big = H.arguments((3, 128, 60, 50, 3), H.ROTATION[0])
    small = _prefix(big, 127)
    assert H.route(*small.case)[0] == 'lds' and H.route(*big.case)[0] == 'simple'
    (P1, o1), (P2, o2) = launch(k, small, backward=False), launch(k, big, backward=False)
    torch.cuda.synchronize()
    P1.check(), P2.check()
    for name in ('z', 'keep', 'h', 'logits'):
        assert same_bits(o1[name], o2[name][:127]), name


def test_backward_rows_do_not_depend_on_the_route():
    """dloss NULL, dlogits_ext set: rows 0..163 of every dx from B = 164 (k_head_bwd) and from B = 165 (k_head_bwd_simple)."""
    k = hip()
    big = H.arguments((3, 165, 60, 50, 3), H.Form(1, True, 'valid', 'ext', 0.2, 'normal'))
    small = _prefix(big, 164)
    assert H.route(*small.case)[1] == 'lds' and H.route(*big.case)[1] == 'simple'
    (P1, o1), (P2, o2) = launch(k, small), launch(k, big)
    torch.cuda.synchronize()
    P1.check(), P2.check()
    for s in range(3):
        assert same_bits(o1['dx'][s], o2['dx'][s][:164]), 'dx[%d]' % s
    assert same_bits(o1['z'], o2['z'][:164]) and same_bits(o1['logits'], o2['logits'][:164])


# ---------------------------------------------------------------------------------------------- corrupt labels, refusals
@pytest.mark.parametrize('label', ['L', -1])
@pytest.mark.parametrize('case', [H.BASE, (3, 165, 60, 50, 3), (3, 1, 64, 196, 5)])
def test_a_corrupt_label_poisons_the_step(case, label):
    """Finite logits; NaN in the loss and in every element of every gradient -- also when the corrupt label is the only one (B = 1)."""
    k = hip()
    a = H.arguments(case, H.ROTATION[0])
    a.y = a.y.clone()
    a.y[a.B // 2] = a.L if label == 'L' else label
    P, o = launch(k, a)
    torch.cuda.synchronize()
    P.check()
    assert bool(torch.isfinite(o['logits']).all()) and bool(torch.isnan(o['loss']).all())
    for name in ('dW1', 'db1', 'dW2', 'db2'):
        assert bool(torch.isnan(o[name]).all()), name
    assert all(bool(torch.isnan(d).all()) for d in o['dx'])
    ref = H.compute(a)
    ex = H.Excess()
    H.judge_forward(a, ref, o, ex)
    H.judge_backward(a, ref, o, ex)
    assert all(e <= 1.0 for e in ex.values()), ex.line()


def _untouched(P):
    for buf, _ in P.watch:
        got = buf.cpu()
        assert torch.equal(got, torch.full_like(got, H.CANARY)), 'a refusing entry point wrote to an output'


def test_entries_refuse_what_they_cannot_run():
    """nseg 0 and 4, B, D, H1 or L of 0, and drop_p of 1.0 or negative: a non-zero return and no output touched."""
    k = hip()
    a = H.arguments(H.BASE, H.ROTATION[0])
    Pok, f = launch(k, a, backward=False)
    nseg, B, D, H1, L = H.BASE
    bad_dims = [(0, B, D, H1, L), (4, B, D, H1, L), (nseg, 0, D, H1, L), (nseg, B, 0, H1, L), (nseg, B, D, 0, L), (nseg, B, D, H1, 0)]
    P = H.Place(DEV)
    for dims in bad_dims:
        assert H.run_forward(k, P, a, dims=dims)['rc'] != 0, dims
        assert H.run_backward(k, P, a, f, dims=dims)['rc'] != 0, dims
    for p in (1.0, -0.25):
        assert H.run_forward(k, P, a, drop_p=p)['rc'] != 0, p
    torch.cuda.synchronize()
    assert len(P.watch) == 6 * (3 + 2 + 3) + 2 * 3
    _untouched(P)
    Pok.check()


# ---------------------------------------------------------------------------------------------- the autograd wrapper
def _on_device(a):
    d = H.Bag(xs=[x.to(DEV).requires_grad_() for x in a.xs], W1=a.W1.to(DEV).requires_grad_(), W2=a.W2.to(DEV).requires_grad_(),
              b1=None if a.b1 is None else a.b1.to(DEV).requires_grad_(), b2=None if a.b2 is None else a.b2.to(DEV).requires_grad_())
    d.cfg = dict(act=a.act, drop_p=a.p, seed=a.seed, labels=a.y.to(DEV), owner=None)
    return d


@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('case', [H.BASE, (3, 165, 60, 50, 3)])
def test_wrapper_gives_the_bits_of_the_direct_call(case, bias):
    """native._Head.apply: logits, loss and every gradient equal the direct call's bits; without biases it returns no db1 / db2."""
    k = hip()
    a = H.arguments(case, H.Form(1, bias, 'valid', 'both', 0.2, 'normal'))
    P, o = launch(k, a)
    d = _on_device(a)
    logits, loss = native._Head.apply(d.cfg, d.W1, d.b1, d.W2, d.b2, *d.xs)
    node = logits.grad_fn
    got = native._Head.backward(node, a.ext.to(DEV), torch.tensor(a.dloss, device=DEV))
    torch.cuda.synchronize()
    P.check()
    assert same_bits(logits, o['logits']) and same_bits(loss.reshape(1), o['loss'])
    assert len(got) == 5 + a.nseg and got[0] is None
    assert same_bits(got[1], o['dW1']) and same_bits(got[3], o['dW2'])
    if bias:
        assert same_bits(got[2], o['db1']) and same_bits(got[4], o['db2'])
    else:
        assert got[2] is None and got[4] is None
    for s in range(a.nseg):
        assert same_bits(got[5 + s], o['dx'][s]), 'dx[%d]' % s
    # and through autograd itself
    (0.75 * loss + (logits * a.ext.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert same_bits(d.W1.grad, o['dW1']) and same_bits(d.W2.grad, o['dW2'])
    assert all(same_bits(x.grad, o['dx'][s]) for s, x in enumerate(d.xs))
    if bias:
        assert same_bits(d.b1.grad, o['db1']) and same_bits(d.b2.grad, o['db2'])


def test_native_head_without_biases_leaky_one_readout():
    """native.head over Sequential(Linear(bias=False), LeakyReLU, Linear(bias=False)) and ONE readout against the same modules run
    in float64 on the CPU, under the yardstick of this file."""
    hip()
    case = (1, 33, 21, 13, 4)
    form = H.Form(3, False, 'two', 'dloss', 0.0, 'normal')
    a = H.arguments(case, form)
    ref = H.compute(a)
    stack = torch.nn.Sequential(torch.nn.Linear(a.K, a.H1, bias=False), torch.nn.LeakyReLU(), torch.nn.Linear(a.H1, a.L, bias=False))
    with torch.no_grad():
        stack[0].weight.copy_(a.W1), stack[2].weight.copy_(a.W2)
    wide = copy.deepcopy(stack).double()
    x64 = a.xs[0].double().requires_grad_()
    logits64 = wide(x64)
    loss64 = F.cross_entropy(logits64, a.y)
    loss64.backward()
    stack = stack.to(DEV)
    x = a.xs[0].to(DEV).requires_grad_()
    out = native.head(stack, [x], a.y.to(DEV), True)
    assert out is not None, 'native.head does not cover the stack'
    logits, loss = out
    loss.backward()
    ex = H.Excess()
    ex.add('logits', H.excess_terms(logits, logits64.detach(), ref.t_logits))
    ex.add('loss', H.excess_terms(loss, loss64.detach(), ref.t_loss))
    g = 1.0 / a.dloss                                  # the reference's terms are those of dloss = head_ref.DLOSS; here dloss is 1
    ex.add('dW1', H.excess_terms(stack[0].weight.grad, wide[0].weight.grad, g * ref.t_dW1))
    ex.add('dW2', H.excess_terms(stack[2].weight.grad, wide[2].weight.grad, g * ref.t_dW2))
    ex.add('dx', H.excess_terms(x.grad, x64.grad, g * ref.t_dx[0]))
    print('HEAD native.head: ' + ex.line())
    assert all(e <= 1.0 for e in ex.values()), ex.line()


# ---------------------------------------------------------------------------------------------- the model past both boundaries
@pytest.mark.parametrize('graphs', [130, 170])
def test_model_head_past_the_lds_boundaries(graphs):
    """130 graphs (simple forward, LDS backward) and 170 graphs (both simple) of about 40 nodes through SoftPoolingGcnEncoder: the
    native head against the module stack, as test_native_gpu.test_fused_head_matches_the_module_stack builds it and to its bars."""
    from test_native_gpu import _pair
    assert H.route(3, 130, 60, 50, 3) == ('simple', 'lds') and H.route(3, 170, 60, 50, 3) == ('simple', 'simple')
    ds = SyntheticCellGraphs(graphs, 40, num_features=16, base_seed=2)
    b = Batch.from_data_list([ds[i] for i in range(graphs)]).to(DEV)
    kw = dict(concat=True, load_data_sparse=True, drop_out=0.)       # without DenseJK the three readouts are 60 wide: K = 180
    nat, ref = _pair((600, 16, 20, 20, True, True, 20, 3, 0.1, [50]), kw, head=True)
    ref.native = True                                  # same levels; only the head differs
    ref.native_head = False
    assert nat.native_head
    assert nat.pred_model[0].in_features == 180 and nat.pred_model[0].out_features == 50 and nat.pred_model[-1].out_features == 3
    ln, lossn = nat(b)
    lr, lossr = ref(b)
    assert ln.shape == (graphs, 3)
    lossn.backward()
    lossr.backward()
    def rel(x, y):
        x, y = x.detach().double(), y.detach().double()
        return float((x - y).abs().max() / (y.abs().max() + 1e-30))
    print('HEAD model B=%d: logits %.3g loss %.3g' % (graphs, rel(ln, lr), rel(lossn, lossr)))
    assert rel(ln, lr) < 2e-6 and rel(lossn, lossr) < 2e-6
    gr = dict(ref.named_parameters())
    for name, p in nat.named_parameters():
        if name.startswith('pred_model'):
            print('HEAD model B=%d: grad %s %.3g' % (graphs, name, rel(p.grad, gr[name].grad)))
            assert rel(p.grad, gr[name].grad) < 5e-6, (name, rel(p.grad, gr[name].grad))


def test_case_list_is_the_one_of_the_cpu_file():
    assert [H.BASE] + OTHER_CASES == list(H.CASES)
