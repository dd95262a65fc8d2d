"""GPU: cgc_net_amd.optim.SGD / RMSprop against torch.optim.SGD(fused=True) / torch.optim.RMSprop(foreach=True), on the model
the Adam tests of test_native_gpu.py use.  Both levels -- cached lists calling torch's kernels, and ONE launch of cgc_sgd_step /
cgc_rmsprop_step on the step sequencer's flat gradient buffers -- must give the same parameters and optimiser state BIT FOR BIT:
the kernels evaluate torch's arithmetic in torch's order with torch's FMA contractions (csrc/optim.hip).  The number of one-launch
steps is counted at the call, so a silent fall-back cannot pass for the kernel."""
import copy
import os

import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import network
from cgc_net_amd.data import Batch, SyntheticCellGraphs
from cgc_net_amd.optim import SGD, RMSprop, init_optim

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARGS = (400, 16, 20, 20, True, True, 20, 3, 0.1, [50])
KW = dict(concat=True, load_data_sparse=True, norm_adj=True, jk=True)


def _models(n, args=ARGS, seed=5):
    torch.manual_seed(seed)
    ms = [network.SoftPoolingGcnEncoder(*args, **KW).to(DEV) for _ in range(n)]
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    for m in ms:
        m.native, m.native_head = True, True
    return [m.train() for m in ms]


def _batch(seed, nodes=200):
    ds = SyntheticCellGraphs(4, nodes, num_features=16, base_seed=seed)
    return Batch.from_data_list([ds[i] for i in range(4)]).to(DEV)


def _ours(name, model, one_launch=True, momentum=0.9, grad_mul=1.0):
    if name == 'sgd':
        o = SGD(model.parameters(), lr=1e-2, momentum=momentum, weight_decay=1e-4, model=model if one_launch else None,
                grad_mul=grad_mul)
    else:
        o = RMSprop(model.parameters(), lr=1e-3, momentum=momentum, weight_decay=1e-4, model=model if one_launch else None,
                    grad_mul=grad_mul)
    o.launches = 0
    launch = o._launch

    def counted(*a):
        o.launches += 1
        return launch(*a)
    o._launch = counted
    return o


def _torch(name, model, momentum=0.9):
    if name == 'sgd':
        return torch.optim.SGD(model.parameters(), lr=1e-2, momentum=momentum, weight_decay=1e-4, fused=True)
    return torch.optim.RMSprop(model.parameters(), lr=1e-3, momentum=momentum, weight_decay=1e-4, foreach=True)


def _fwd_bwd(m, o, b, passes=1):
    o.zero_grad()
    for _ in range(passes):
        _, loss = m(b)
        loss.backward()


def _assert_same(a, c, oa, oc):
    for (k, p), (_, q) in zip(a.state_dict().items(), c.state_dict().items()):
        assert torch.equal(p, q), k
    sa, sc = oa.state_dict()['state'], oc.state_dict()['state']
    assert sa.keys() == sc.keys()
    for i in sc:
        assert sa[i].keys() == sc[i].keys(), i
        for key, v in sc[i].items():
            assert torch.equal(sa[i][key], v), (i, key)


@pytest.mark.parametrize('one_launch', [False, True], ids=['lists', 'one_launch'])
@pytest.mark.parametrize('name', ['sgd', 'rmsprop'])
def test_equals_torch_bitwise(name, one_launch):
    """7 steps with a StepLR schedule (the LR changes after step 3 and 6) and a step whose gradients were accumulated over two
    backward passes (step 4: not where the sequencer leaves them, so torch's kernels take it)."""
    b = _batch(9)
    a, c = _models(2)
    oa, oc = _ours(name, a, one_launch), _torch(name, c)
    sched = [torch.optim.lr_scheduler.StepLR(o, step_size=3, gamma=0.5) for o in (oa, oc)]
    for step in range(7):
        for m, o in ((a, oa), (c, oc)):
            _fwd_bwd(m, o, b, 2 if step == 4 else 1)
            o.step()
        for s in sched:
            s.step()
    assert oa.param_groups[0]['lr'] == oc.param_groups[0]['lr'] < oc.defaults['lr']
    assert oa.launches == (5 if one_launch else 0)            # steps 1, 2, 3, 5, 6 (0 creates the state, 4 accumulates)
    _assert_same(a, c, oa, oc)


@pytest.mark.parametrize('name', ['sgd', 'rmsprop'])
def test_checkpoint_resume_both_directions(name):
    """ours (3 one-launch-era steps) -> torch's class -> ours again, through evalio's checkpoint dict: the trajectory of an
    uninterrupted torch run, step counts included."""
    from cgc_net_amd import evalio
    b = _batch(11)
    a, c = _models(2)
    oc = _torch(name, c)
    for _ in range(7):
        _fwd_bwd(c, oc, b)
        oc.step()
    oa = _ours(name, a)
    for _ in range(3):
        _fwd_bwd(a, oa, b)
        oa.step()
    ck = evalio.checkpoint_state(a, oa, 0, 0.0, 0.0)
    ot = _torch(name, a)
    ot.load_state_dict(ck['optimizer'])
    for _ in range(2):
        _fwd_bwd(a, ot, b)
        ot.step()
    oa2 = _ours(name, a)
    oa2.load_state_dict(ot.state_dict())
    for _ in range(2):
        _fwd_bwd(a, oa2, b)
        oa2.step()
    assert oa.launches == 2 and oa2.launches == 1          # (after a load the first step rebuilds the lists on torch's path)
    _assert_same(a, c, oa2, oc)
    if name == 'rmsprop':
        assert all(float(st['step']) == 7.0 for st in oa2.state_dict()['state'].values())


@pytest.mark.parametrize('name', ['sgd', 'rmsprop'])
def test_notices_moved_parameters(name):
    b = _batch(12)
    a, c = _models(2)
    oa, oc = _ours(name, a), _torch(name, c)
    launched = []
    for step in range(6):
        if step == 3:
            for m in (a, c):
                m.to('cpu')
                m.to(DEV)
        n = oa.launches
        for m, o in ((a, oa), (c, oc)):
            _fwd_bwd(m, o, b)
            o.step()
        launched.append(oa.launches - n)
    assert launched == [0, 1, 1, 0, 1, 1]
    _assert_same(a, c, oa, oc)


@pytest.mark.parametrize('name', ['sgd', 'rmsprop'])
def test_parameter_frozen_mid_training_then_thawed(name):
    """A parameter without a gradient is not touched by torch; the sequencer still writes its slice of the flat buffer, so those
    steps are torch's.  After the thaw the one-launch path resumes (neither rule reads a step count)."""
    b = _batch(14)
    a, c = _models(2)
    oa, oc = _ours(name, a), _torch(name, c)
    launched, frozen_before = [], None
    for step in range(8):
        if step == 3:
            for m in (a, c):
                m.GCN_embed_2.gcn2.weight.requires_grad_(False)
            frozen_before = a.GCN_embed_2.gcn2.weight.detach().clone()
        if step == 5:
            for m in (a, c):
                m.GCN_embed_2.gcn2.weight.requires_grad_(True)
        n = oa.launches
        for m, o in ((a, oa), (c, oc)):
            _fwd_bwd(m, o, b)
            o.step()
        launched.append(oa.launches - n)
        if step == 4:
            assert torch.equal(a.GCN_embed_2.gcn2.weight, frozen_before)
    assert launched == [0, 1, 1, 0, 0, 0, 1, 1], launched
    _assert_same(a, c, oa, oc)


@pytest.mark.parametrize('name', ['sgd', 'rmsprop'])
def test_gradient_scale(name):
    b = _batch(13)
    a, c = _models(2)
    oa, oc = _ours(name, a, grad_mul=0.25), _torch(name, c)
    for step in range(4):
        for m, o in ((a, oa), (c, oc)):
            _fwd_bwd(m, o, b)
            if o is oc:
                torch._foreach_mul_([p.grad for p in c.parameters()], 0.25)
            o.step()
    assert oa.launches == 3
    _assert_same(a, c, oa, oc)


@pytest.mark.parametrize('name', ['sgd', 'rmsprop'])
def test_without_momentum(name):
    """momentum 0: SGD keeps no state at all (both table columns NULL), RMSprop only square_avg."""
    b = _batch(15)
    a, c = _models(2)
    oa, oc = _ours(name, a, momentum=0.0), _torch(name, c, momentum=0.0)
    for _ in range(5):
        for m, o in ((a, oa), (c, oc)):
            _fwd_bwd(m, o, b)
            o.step()
    assert oa.launches == 4
    _assert_same(a, c, oa, oc)


@pytest.mark.parametrize('name', ['sgd', 'rmsprop'])
def test_shipped_widths(name):
    """C1 = 1140 (the shipped configuration): the table covers the large parameter tensors."""
    b = _batch(3, nodes=600)
    a, c = _models(2, args=(11404, 16, 20, 20, True, True, 20, 3, 0.1, [50]))
    oa, oc = _ours(name, a), _torch(name, c)
    for _ in range(3):
        for m, o in ((a, oa), (c, oc)):
            _fwd_bwd(m, o, b)
            o.step()
    assert oa.launches == 2
    assert max(p.numel() for p in a.parameters()) > 1024 * 256
    _assert_same(a, c, oa, oc)


@pytest.mark.parametrize('name', ['sgd', 'rmsprop'])
def test_one_launch_under_data_parallel(name):
    """parallel.DataParallel on a one-rank RCCL group, the optimiser built the way the reference's train.py does (init_optim with the
    module): the second step is one launch, and it equals torch's optimiser stepping from the same state and gradients."""
    import torch.distributed as dist
    from cgc_net_amd.parallel import DataParallel
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(29700 + os.getpid() % 1000))
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        b = _batch(21)
        net, ref = _models(2)
        dp = DataParallel(net)
        opt = init_optim(name, dp.module.parameters(), 1e-2 if name == 'sgd' else 1e-3, 1e-4, model=dp.module)
        calls = []
        launch = opt._launch
        opt._launch = lambda *a: (calls.append(1), launch(*a))[1]
        for step in range(2):
            opt.zero_grad()
            _, loss = dp(b)
            torch.mean(loss).backward()
            if step == 1:
                ref.load_state_dict(net.state_dict())
                for p, q in zip(ref.parameters(), net.parameters()):
                    p.grad = q.grad.clone()
                kw = dict(fused=True) if name == 'sgd' else dict(foreach=True)
                oref = getattr(torch.optim, 'SGD' if name == 'sgd' else 'RMSprop')(ref.parameters(), lr=1.0, **kw)
                oref.load_state_dict(copy.deepcopy(opt.state_dict()))     # (a load keeps tensors already in place: not shared)
                oref.step()
            opt.step()
        assert len(calls) == 1
        _assert_same(net, ref, opt, oref)
    finally:
        dist.destroy_process_group()
