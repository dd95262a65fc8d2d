"""CPU: init_optim maps the reference's names (common/utils.py:119-127) to cgc_net_amd.optim's classes; SGD and RMSprop on host tensors
follow torch's own optimisers through the cached-list level (there are no flat gradient buffers, so the one-launch path is never
taken); their state_dicts move between these classes and torch's in both directions."""
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd.optim import SGD, Adam, RMSprop, init_optim

KINDS = {
    'sgd': (SGD, lambda ps: torch.optim.SGD(ps, lr=1e-2, momentum=0.9, weight_decay=1e-4)),
    'rmsprop': (RMSprop, lambda ps: torch.optim.RMSprop(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4)),
}


def _ours(name, ps, model=None, grad_mul=1.0):
    cls = KINDS[name][0]
    lr = 1e-2 if name == 'sgd' else 1e-3
    return cls(ps, lr=lr, momentum=0.9, weight_decay=1e-4, model=model, grad_mul=grad_mul)


def test_init_optim_maps_the_reference_names():
    m = torch.nn.Linear(3, 2)
    o = init_optim('adam', m.parameters(), 1e-3, 1e-4, model=m)
    assert type(o) is Adam and o.param_groups[0]['lr'] == 1e-3 and o.param_groups[0]['weight_decay'] == 1e-4 and o._model is m
    o = init_optim('sgd', m.parameters(), 1e-2, 1e-4)
    g = o.param_groups[0]
    assert type(o) is SGD and (g['lr'], g['momentum'], g['weight_decay'], g['dampening'], g['nesterov']) == (1e-2, 0.9, 1e-4, 0, False)
    o = init_optim('rmsprop', m.parameters(), 1e-3, 1e-4, model=m)
    g = o.param_groups[0]
    assert type(o) is RMSprop and o._model is m
    assert (g['lr'], g['momentum'], g['weight_decay'], g['alpha'], g['eps'], g['centered']) == (1e-3, 0.9, 1e-4, 0.99, 1e-8, False)
    with pytest.raises(KeyError, match='Unsupported optim: adamw'):
        init_optim('adamw', m.parameters(), 1e-3, 1e-4)


@pytest.mark.parametrize('name', list(KINDS))
def test_host_trajectory_equals_torch(name):
    torch.manual_seed(0)
    a, b = torch.nn.Linear(5, 3), torch.nn.Linear(5, 3)
    b.load_state_dict(a.state_dict())
    oa = _ours(name, a.parameters(), model=a)
    ob = KINDS[name][1](b.parameters())
    x = torch.randn(7, 5)
    for _ in range(5):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            m(x).pow(2).sum().backward()
            o.step()
    assert oa._lists is not None and not oa._fast_ready()
    for (k, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.allclose(p, q, atol=1e-7), k
    sa, sb = oa.state_dict()['state'], ob.state_dict()['state']
    for i in sb:
        for key, v in sb[i].items():
            assert torch.allclose(sa[i][key], v, atol=1e-7), (i, key)


@pytest.mark.parametrize('name', list(KINDS))
def test_host_late_gradients_and_grad_mul(name):
    """A parameter whose first gradient arrives on a later step, and one that misses a step, with grad_mul: torch's trajectory on
    gradients scaled beforehand, and the caller's p.grad untouched."""
    class Two(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(4, 3), torch.nn.Linear(4, 3)

        def forward(self, x, use_b):
            return self.a(x) + (self.b(x) if use_b else 0.0)
    torch.manual_seed(0)
    m, r = Two(), Two()
    r.load_state_dict(m.state_dict())
    b0 = m.b.weight.detach().clone()
    om = _ours(name, m.parameters(), model=m, grad_mul=0.5)
    orr = KINDS[name][1](r.parameters())
    x = torch.randn(6, 4)
    for step in range(7):
        use_b = step >= 2 and step != 4
        for mod, o in ((m, om), (r, orr)):
            o.zero_grad()
            mod(x, use_b).pow(2).sum().backward()
        before = [p.grad.clone() if p.grad is not None else None for p in m.parameters()]
        for p in r.parameters():
            if p.grad is not None:
                p.grad.mul_(0.5)
        om.step()
        orr.step()
        for p, g in zip(m.parameters(), before):
            assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
    for (k, p), (_, q) in zip(m.state_dict().items(), r.state_dict().items()):
        assert torch.allclose(p, q, atol=1e-7), k
    assert float((m.b.weight.detach() - b0).abs().max()) > 1e-4
    if name == 'rmsprop':
        steps = [float(st['step']) for st in om.state_dict()['state'].values()]
        assert steps == [7.0, 7.0, 4.0, 4.0], steps


@pytest.mark.parametrize('name', list(KINDS))
def test_state_dict_interchange_with_torch(name):
    """torch's optimiser -> ours -> torch's: three optimisers in a row continue one trajectory."""
    torch.manual_seed(1)
    a, b = torch.nn.Linear(5, 3), torch.nn.Linear(5, 3)
    b.load_state_dict(a.state_dict())
    x = torch.randn(7, 5)

    def run(m, o, n):
        for _ in range(n):
            o.zero_grad()
            m(x).pow(2).sum().backward()
            o.step()
    ref = KINDS[name][1](a.parameters())
    run(a, ref, 9)                                   # uninterrupted
    t1 = KINDS[name][1](b.parameters())
    run(b, t1, 3)
    ours = _ours(name, b.parameters(), model=b)
    ours.load_state_dict(t1.state_dict())
    run(b, ours, 3)
    t2 = KINDS[name][1](b.parameters())
    t2.load_state_dict(ours.state_dict())
    run(b, t2, 3)
    for (k, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.allclose(p, q, atol=1e-7), k
    if name == 'rmsprop':
        assert all(float(st['step']) == 9.0 for st in t2.state_dict()['state'].values())
