"""GPU: the DiffPool regularisers (``SoftPoolingGcnEncoder(diffpool_loss=True)``: ``link_loss`` / ``ent_loss``, csrc/diffpool_reg.hip).

* against float64: the dense oracle (oracle/dense_ref.py) in float64 with its ``diff_pool`` wrapped to also compute PyG
  dense_diff_pool's link / entropy losses from its own (adj, s, mask) -- values to 1e-5, gradients to 1e-4 of the largest float64
  entry, in every GEMM mode with every product on the 128 x 128 route;
* the step sequencer (native.level / level_eval) against the per-operator path (ops._DiffPoolReg);
* the flag alone changes nothing (bitwise), the step is deterministic, saved tensors are not modified;
* the benchmarked C3 batch against a float64 restatement computed from the model's own S and graph."""
import pytest
import torch

import cgc_net_amd  # noqa: F401
from cgc_net_amd import network
from cgc_net_amd.data import Batch, SyntheticCellGraphs
from oracle import dense_ref
from util import dense_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARGS = (600, 16, 20, 20, True, True, 20, 3, 0.1, [50])        # C1 = 60, C2 = 6


def _pyg_reg(adj, s, mask=None):
    """torch_geometric dense_diff_pool's two regularisers (restated: PyG is not a dependency)."""
    s = torch.softmax(s, dim=-1)
    if mask is not None:
        s = s * mask
    link = torch.norm(adj - torch.matmul(s, s.transpose(1, 2)), p=2) / adj.numel()
    ent = (-s * torch.log(s + 1e-15)).sum(dim=-1).mean()
    return link, ent


def _wrap_oracle(monkeypatch):
    got = dict(link=[], ent=[], numel=[])
    orig = dense_ref.diff_pool

    def diff_pool(x, adj, s, mask=None):
        link, ent = _pyg_reg(adj, s, mask)
        got['link'].append(link)
        got['ent'].append(ent)
        got['numel'].append(adj.numel())
        return orig(x, adj, s, mask)
    monkeypatch.setattr(dense_ref, 'diff_pool', diff_pool)
    return got


def _batch(B=4, nodes=120, seed=11):
    ds = SyntheticCellGraphs(B, nodes, num_features=16, base_seed=seed)
    return Batch.from_data_list([ds[i] for i in range(B)])


def _padded_tuple(cpu_batch, extra=7):
    """The reference's dense tuple input, padded beyond the largest graph."""
    x, adj, counts, y = dense_inputs(cpu_batch, torch.float32)
    B, N, F = x.shape
    xp = torch.zeros(B, N + extra, F)
    ap = torch.zeros(B, N + extra, N + extra)
    xp[:, :N], ap[:, :N, :N] = x, adj
    return xp, ap, counts, y


CASES = {
    'plain': dict(),
    'shipped': dict(norm_adj=True, jk=True),
    'tuple_padded': dict(norm_adj=True, load_data_sparse=False),
    'gin': dict(gcn_name='GIN'),
}


def _kw(flags):
    kw = dict(concat=True, gcn_name='SAGE', load_data_sparse=True, drop_out=0.)
    kw.update(flags)
    return kw


def _inputs(name):
    cpu = _batch()
    if name == 'tuple_padded':
        t = _padded_tuple(cpu)
        return tuple(v.to(DEV) for v in t), (t[0].double(), t[1].double(), t[2], t[3])
    return cpu.to(DEV), dense_inputs(cpu)


def _grads(model, loss):
    model.zero_grad(set_to_none=True)
    loss.backward(retain_graph=True)
    return {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}


@pytest.mark.parametrize('name', list(CASES))
def test_against_float64_oracle(name, gemm_mode, forced_big_route, monkeypatch):
    kw = _kw(CASES[name])
    torch.manual_seed(0)
    ref = dense_ref.SoftPoolingGcnEncoder(*ARGS, **kw).double().train()
    model = network.SoftPoolingGcnEncoder(*ARGS, diffpool_loss=True, **kw)
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    model.to(DEV).train()
    x, x64 = _inputs(name)
    got = _wrap_oracle(monkeypatch)
    ref.load_data_sparse = False                      # the oracle takes the densified float64 tuple
    _, loss64 = ref(x64)
    _, loss = model(x)
    assert len(model.link_loss) == len(model.ent_loss) == 2
    for k in range(2):
        for mine, want in ((model.link_loss[k], got['link'][k]), (model.ent_loss[k], got['ent'][k])):
            assert mine.dim() == 0 and mine.requires_grad
            rel = abs(mine.item() - want.item()) / abs(want.item())
            assert rel < 1e-5, (name, k, mine.item(), want.item(), rel)
    numel = got['numel']
    params64 = dict(ref.named_parameters())
    for what in ('link', 'ent'):
        if what == 'link':
            mine = sum(n * v for n, v in zip(numel, model.link_loss))
            want = sum(n * v for n, v in zip(numel, got['link']))
        else:
            mine, want = sum(model.ent_loss), sum(got['ent'])
        g = _grads(model, mine)
        ref.zero_grad(set_to_none=True)
        want.backward(retain_graph=True)
        scale = max(p.grad.abs().max().item() for p in params64.values() if p.grad is not None)
        for k, p64 in params64.items():
            g64 = p64.grad if p64.grad is not None else torch.zeros_like(p64)
            err = (g[k].cpu().double() - g64).abs().max().item()
            top = g64.abs().max().item()
            # the bar is 1e-4 of the tensor's largest float64 entry.  A tensor whose float64 gradient is zero up to rounding (below
            # 1e-6 of the model's largest gradient: DenseJK's attention bias, to which the softmax over layers is invariant) has no
            # scale of its own; it is held to 1e-7 of the model's largest gradient (measured: at most 7.3e-9 of it)
            bar = 1e-4 * top if top >= 1e-6 * scale else 1e-7 * scale
            assert err <= bar, (name, gemm_mode.name, what, k, err, top, scale)
    gemm_mode.check_applied(1)


def _spy(monkeypatch, attr):
    calls = []
    orig = getattr(network.native, attr)

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(network.native, attr, spy)
    return calls


def _pair(flags, seed=5):
    kw = _kw(flags)
    torch.manual_seed(seed)
    a = network.SoftPoolingGcnEncoder(*ARGS, diffpool_loss=True, **kw).to(DEV)
    b = network.SoftPoolingGcnEncoder(*ARGS, diffpool_loss=True, **kw).to(DEV)
    b.load_state_dict(a.state_dict())
    a.native, b.native = True, False
    return a.train(), b.train()


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _check_grads(gn, go, rtol, what):
    """Per tensor: max|gn - go| <= rtol max|go|.  A tensor whose gradient is zero up to rounding (below 1e-6 of the model's largest:
    DenseJK's attention bias, to which the softmax over layers is invariant) is held to rtol of the model's largest gradient: its
    values are the rounding residue of terms of that size, summed in another order."""
    scale = max(g.abs().max().item() for g in go.values())
    for k in gn:
        err, top = (gn[k].double() - go[k].double()).abs().max().item(), go[k].abs().max().item()
        bar = rtol * top if top >= 1e-6 * scale else rtol * scale
        assert err <= bar, (what, k, err, top, scale)


@pytest.mark.parametrize('mode', ['0', '2'])
@pytest.mark.parametrize('name', ['plain', 'shipped'])
def test_sequencer_equals_per_operator_path(name, mode, monkeypatch):
    monkeypatch.setenv('CGC_GEMM_16BIT', mode)
    nat, ops_ = _pair(CASES[name])
    x = _batch(B=5, nodes=200, seed=3).to(DEV)
    calls = _spy(monkeypatch, 'level')
    _, loss_n = nat(x)
    assert len(calls) == 3
    _, loss_o = ops_(x)
    assert len(calls) == 3                            # the per-operator model did not go through the sequencer
    for k in range(2):
        assert _rel(nat.link_loss[k], ops_.link_loss[k]) < 2e-6
        assert _rel(nat.ent_loss[k], ops_.ent_loss[k]) < 2e-6
    C1 = nat.GCN_pool_1.gcn3.out_channels
    g = nat.last_graph
    numel = [g.B * g.npad * g.npad, g.B * C1 * C1]
    objectives = [lambda m: sum(n * v for n, v in zip(numel, m.link_loss)), lambda m: sum(m.ent_loss),
                  lambda m: None]
    for obj in objectives:
        ln, lo = obj(nat), obj(ops_)
        if ln is None:
            ln, lo = loss_n + sum(nat.link_loss) + sum(nat.ent_loss), loss_o + sum(ops_.link_loss) + sum(ops_.ent_loss)
        _check_grads(_grads(nat, ln), _grads(ops_, lo), 2e-6, (name, mode))
    # eval under no_grad: level_eval on the sequencer
    nat.eval()
    ops_.eval()
    ev = _spy(monkeypatch, 'level_eval')
    with torch.no_grad():
        nat(x)
        assert len(ev) == 3
        ops_(x)
        assert len(ev) == 3
    for k in range(2):
        assert not nat.link_loss[k].requires_grad
        assert _rel(nat.link_loss[k], ops_.link_loss[k]) < 2e-6
        assert _rel(nat.ent_loss[k], ops_.ent_loss[k]) < 2e-6


@pytest.mark.parametrize('native', [True, False])
@pytest.mark.parametrize('mode', ['0', '1', '2'])
def test_flag_alone_changes_nothing(native, mode, monkeypatch):
    monkeypatch.setenv('CGC_GEMM_16BIT', mode)
    kw = _kw(CASES['shipped'])
    torch.manual_seed(7)
    off = network.SoftPoolingGcnEncoder(*ARGS, **kw).to(DEV).train()
    on = network.SoftPoolingGcnEncoder(*ARGS, diffpool_loss=True, **kw).to(DEV).train()
    on.load_state_dict(off.state_dict())
    off.native = on.native = native
    assert list(off.state_dict().keys()) == list(on.state_dict().keys())
    x = _batch(B=4, nodes=150, seed=9).to(DEV)
    lo, loss_off = off(x)
    ln, loss_on = on(x)
    assert off.link_loss == [] and off.ent_loss == [] and len(on.link_loss) == 2
    assert torch.equal(lo, ln) and torch.equal(loss_off, loss_on)
    loss_off.backward()
    loss_on.backward()
    go, gn = dict(off.named_parameters()), dict(on.named_parameters())
    for k in go:
        assert torch.equal(go[k].grad, gn[k].grad), k
    on.diffpool_loss = False                          # switched off later: lists empty again, same results
    ln2, _ = on(x)
    assert on.link_loss == [] and on.ent_loss == [] and torch.equal(ln2, lo)


@pytest.mark.parametrize('native', [True, False])
def test_deterministic_and_saved_tensors_untouched(native):
    kw = _kw(CASES['shipped'])
    torch.manual_seed(3)
    m = network.SoftPoolingGcnEncoder(*ARGS, diffpool_loss=True, **kw).to(DEV).train()
    m.native = native
    x = _batch(B=4, nodes=150, seed=4).to(DEV)
    res = []
    for _ in range(2):
        _, cls = m(x)
        loss = cls + sum(m.link_loss) * 1e4 + sum(m.ent_loss)
        g1 = _grads(m, loss)
        g2 = _grads(m, loss)                          # second backward over the same graph (retain_graph)
        for k in g1:
            assert torch.equal(g1[k], g2[k]), k
        res.append((loss.detach().clone(), g1))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_full_size_c3_against_float64_restatement(monkeypatch):
    """The benchmarked C3 batch (32 graphs of ~1800 nodes, max_num_nodes = 11404: C1 = 1140, C2 = 114, shipped flags), exact mode."""
    monkeypatch.setenv('CGC_GEMM_16BIT', '0')
    kw = _kw(dict(norm_adj=True, jk=True, collect_assign=True))
    torch.manual_seed(0)
    nat = network.SoftPoolingGcnEncoder(11404, 16, 20, 20, True, True, 20, 3, 0.1, [50], diffpool_loss=True, **kw).to(DEV).train()
    ds = SyntheticCellGraphs(32, 1800, 16, base_seed=0)
    x = Batch.from_data_list([ds[i] for i in range(32)]).to(DEV)
    calls = _spy(monkeypatch, 'level')
    _, cls = nat(x)
    assert len(calls) == 3
    g = nat.last_graph
    S1, S2 = nat.assign_matrix[0].double(), nat.assign_matrix[1].double()        # [B, npad, C1] (padding rows 1/C1), [B, C1, C2]
    B, npad, C1 = S1.shape
    rowptr, col = g.rowptr.long(), g.col.long()
    nnz = int(rowptr[g.n])
    rows = torch.repeat_interleave(torch.arange(g.n, device=DEV), rowptr[1:g.n + 1] - rowptr[:g.n])
    val = g.val[:nnz].double() if g.val is not None else torch.ones(nnz, dtype=torch.float64, device=DEV)
    sq, ent1, Ap = 0.0, 0.0, torch.empty(B, C1, C1, dtype=torch.float64, device=DEV)
    for b in range(B):
        lo, hi = g.gptr_host[b], g.gptr_host[b + 1]
        sel = (rows >= lo) & (rows < hi)
        A = torch.zeros(hi - lo, hi - lo, dtype=torch.float64, device=DEV)
        A[rows[sel] - lo, col[:nnz][sel] - lo] = val[sel]
        S = S1[b, :hi - lo]
        sq += ((A - S @ S.t()) ** 2).sum().item()
        ent1 += (-S * torch.log(S + 1e-15)).sum().item()
        Ap[b] = S.t() @ (A @ S)
    link1, ent1 = sq ** 0.5 / (B * npad * npad), ent1 / (B * npad)
    At = dense_ref.re_norm_adj(Ap, 0.4, None)
    link2, ent2 = _pyg_reg(At, torch.log(S2))
    for mine, want in ((nat.link_loss[0], link1), (nat.ent_loss[0], ent1), (nat.link_loss[1], link2.item()),
                       (nat.ent_loss[1], ent2.item())):
        assert abs(mine.item() - want) / abs(want) < 1e-5, (mine.item(), want)
    # gradients: sequencer against the per-operator path at full size
    ops_ = network.SoftPoolingGcnEncoder(11404, 16, 20, 20, True, True, 20, 3, 0.1, [50], diffpool_loss=True, **kw).to(DEV).train()
    ops_.load_state_dict(nat.state_dict())
    ops_.native = False
    torch.manual_seed(0)
    _, cls_o = ops_(x)
    numel = [B * npad * npad, B * C1 * C1]
    ln = sum(n * v for n, v in zip(numel, nat.link_loss)) + sum(nat.ent_loss)
    lo_ = sum(n * v for n, v in zip(numel, ops_.link_loss)) + sum(ops_.ent_loss)
    _check_grads(_grads(nat, ln), _grads(ops_, lo_), 2e-6, 'C3')
