"""CPU: the float64 reference of tests/head_ref.py against autograd through nn.Linear / activation / a fixed mask / F.cross_entropy,
its terms, the dispatch restated by head_ref.route() against the table of cases and against the text of csrc/head.hip, the margins
of every input set to the activation kink, the float32 twin under the yardstick of tests/test_head_fp64_gpu.py, the mutants of the
twin (each must be rejected by a factor of 10 or more), and the dropout plane.

e32, the twin's excess, is held to 0.25; an output that cannot meet that in float32 would carry its measured e32 in the table E32
below, and the GPU bound of that output in that case would become max(1, 4 * e32).

    case      output      e32
    (none: the largest e32 over all cases and forms is 0.025, on dl of the base case; dz stays below 0.017, every other
     output below 0.005 -- so every GPU bound is 1)

F.cross_entropy on labels that are all -100 (float64, CPU, reduction 'mean'): the loss is NaN (0 / 0) and the gradient of the
logits is exactly zero everywhere, so every parameter gradient and dx is exactly zero; head_ref.reference returns the same."""
import os

import pytest
import torch
import torch.nn.functional as F

import head_ref as H

# (case, output) -> e32 of the float32 twin, the largest over the forms of that case; absent: e32 <= 0.25
E32 = {
}

HEAD_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'cgc-net_amd', 'csrc', 'head.hip')
KERNELS = (('fwd', 'lds'), ('fwd', 'simple'), ('bwd', 'lds'), ('bwd', 'simple'))


def bound(case, name):
    """The bound of a GPU excess: 1, or 4 x the float32 twin's own excess where the table above records one."""
    return max(1.0, 4.0 * E32.get((case, name), 0.0))


def judged(a, ref, o):
    ex = H.Excess()
    H.judge_forward(a, ref, o, ex)
    H.judge_backward(a, ref, o, ex)
    return ex


# ---------------------------------------------------------------------------------------------- reference against autograd
AUTOGRAD_CASES = [H.BASE, (2, 33, 7, 13, 4), (1, 4, 8, 6, 8), (1, 4, 8, 6, 9), (3, 1, 64, 196, 5), (1, 1, 1, 1, 1)]


def _modules(a):
    xs = [x.double().requires_grad_() for x in a.xs]
    l1 = torch.nn.Linear(a.K, a.H1, bias=a.b1 is not None).double()
    l2 = torch.nn.Linear(a.H1, a.L, bias=a.b2 is not None).double()
    with torch.no_grad():
        l1.weight.copy_(a.W1), l2.weight.copy_(a.W2)
        if a.b1 is not None:
            l1.bias.copy_(a.b1), l2.bias.copy_(a.b2)
    act = {0: lambda t: t, 1: F.relu, 2: F.elu, 3: lambda t: F.leaky_relu(t, 0.01)}[a.act]
    z = l1(torch.cat(xs, 1))
    h = act(z) * a.keep.double()
    return xs, l1, l2, z, h, l2(h)


@pytest.mark.parametrize('case', AUTOGRAD_CASES)
def test_reference_is_autograd_through_the_modules(case):
    close = lambda got, want: float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for form in H.case_forms(case)[::7] if case == H.BASE else H.case_forms(case):
        a = H.arguments(case, form)
        r = H.compute(a)
        xs, l1, l2, z, h, logits = _modules(a)
        assert close(r.z, z.detach()) and close(r.h, h.detach()) and close(r.logits, logits.detach()), (case, form)
        total = None
        if a.y is not None and form.labels != 'ignored':
            loss = F.cross_entropy(logits, a.y)
            per = F.cross_entropy(logits, a.y, reduction='none')
            # (logsumexp - logit_y cancels where one logit dominates: relative to the logits it is the difference of)
            top = 1e-12 * float(logits.detach().abs().max())
            assert float((r.per - per.detach()).abs().max()) <= top and abs(float(r.loss) - float(loss.detach())) <= top, (case, form)
            if a.dloss is not None:
                total = a.dloss * loss
        if a.ext is not None:
            total = (logits * a.ext.double()).sum() + (0.0 if total is None else total)
        got = [r.dW1, r.dW2] + r.dx + ([r.db1, r.db2] if form.bias else [])
        if total is None:                              # nothing flows back: every gradient is exactly zero
            assert all(float(g.abs().max()) == 0.0 for g in got + [r.db1, r.db2, r.dl, r.dz]), (case, form)
            continue
        want = torch.autograd.grad(total, [l1.weight, l2.weight] + xs + ([l1.bias, l2.bias] if form.bias else []))
        for g, w in zip(got, want):
            scale = float(w.abs().max())
            assert float((g - w).abs().max()) <= 1e-12 * scale, (case, form, float((g - w).abs().max()), scale)


def test_all_ignored_labels_are_what_cross_entropy_returns():
    """F.cross_entropy in float64 on the CPU, every label -100: a NaN loss (0 / 0) and an exactly zero gradient; the reference's loss
    is NaN and its gradients are what dlogits_ext alone sends back."""
    form = H.Form(1, True, 'ignored', 'both', 0.2, 'normal')
    a = H.arguments(H.BASE, form)
    xs, l1, l2, z, h, logits = _modules(a)
    loss = F.cross_entropy(logits, a.y)
    assert bool(torch.isnan(loss))
    want = torch.autograd.grad(loss, [logits, l1.weight, l1.bias, l2.weight, l2.bias] + xs, retain_graph=True)
    assert all(float(w.abs().max()) == 0.0 for w in want)
    r = H.compute(a)
    assert bool(torch.isnan(r.loss)) and float(r.per.abs().max()) == 0.0
    assert torch.equal(r.dl, a.ext.double())
    only_ext = H.compute(H.arguments(H.BASE, form._replace(labels='null', grads='ext')))
    for name in ('dW1', 'db1', 'dW2', 'db2'):
        assert torch.equal(getattr(r, name), getattr(only_ext, name)), name
    alone = H.compute(H.arguments(H.BASE, form._replace(grads='dloss')))
    assert bool(torch.isnan(alone.loss))
    assert all(float(g.abs().max()) == 0.0 for g in [alone.dW1, alone.db1, alone.dW2, alone.db2, alone.dl, alone.dz] + alone.dx)


@pytest.mark.parametrize('label', ['L', -1])
def test_a_corrupt_label_poisons_the_reference(label):
    a = H.arguments(H.BASE, H.Form(1, True, 'valid', 'both', 0.2, 'normal'))
    a.y = a.y.clone()
    a.y[5] = a.L if label == 'L' else label
    r = H.compute(a)
    assert bool(torch.isfinite(r.logits).all()) and bool(torch.isnan(r.loss))
    assert all(bool(torch.isnan(g).all()) for g in [r.dW1, r.db1, r.dW2, r.db2] + r.dx)


@pytest.mark.parametrize('case', list(H.CASES))
def test_terms_bound_their_values(case):
    for form in H.case_forms(case):
        r = H.reference_of(case, form)
        pairs = [(r.z, r.t_z), (r.h, r.t_h), (r.logits, r.t_logits), (r.dl, r.t_dl), (r.dz, r.t_dz), (r.dW1, r.t_dW1),
                 (r.db1, r.t_db1), (r.dW2, r.t_dW2), (r.db2, r.t_db2)] + list(zip(r.dx, r.t_dx))
        if r.per is not None:
            pairs.append((r.per, r.t_per))
            if form.labels != 'ignored':
                pairs.append((r.loss, r.t_loss))
        for v, t in pairs:
            assert v.shape == t.shape and bool((t >= v.abs() * (1 - 1e-12)).all()), (case, form)


# ---------------------------------------------------------------------------------------------- dispatch
def test_route_puts_every_case_where_the_table_says():
    for case, want in H.CASES.items():
        assert H.route(*case) == want, (case, H.route(*case), want)
    routes = set(H.CASES.values())
    assert routes == {('lds', 'lds'), ('simple', 'lds'), ('simple', 'simple')}
    # both sides of each boundary, one step apart
    for lo, hi, side in (((3, 127, 60, 50, 3), (3, 128, 60, 50, 3), 0), ((3, 164, 60, 50, 3), (3, 165, 60, 50, 3), 1),
                         ((3, 1, 64, 196, 5), (3, 1, 64, 197, 5), 0), ((3, 40, 300, 50, 3), (3, 41, 300, 50, 3), 1),
                         ((1, 4, 8, 6, 8), (1, 4, 8, 6, 9), 0)):
        assert sum(abs(p - q) for p, q in zip(lo, hi)) == 1
        assert H.route(*lo)[side] == 'lds' and H.route(*hi)[side] == 'simple', (lo, hi)
    # the network's own widths: the forward leaves the LDS kernel at 128 graphs, the backward at 165
    assert [B for B in range(1, 200) if H.route(3, B, 60, 50, 3)[0] == 'simple'][0] == 128
    assert [B for B in range(1, 200) if H.route(3, B, 60, 50, 3)[1] == 'simple'][0] == 165


def test_every_form_meets_every_kernel():
    """Each value of each axis of the argument forms runs on each of the four kernels, outside the base case too; the base case runs
    the full cross."""
    assert len(set(H.case_forms(H.BASE))) == 4 * 2 * 4 * 4 * 3 + 4
    for which, kind in KERNELS:
        seen = {f: set() for f in H.Form._fields}
        for case, rt in H.CASES.items():
            if case == H.BASE or rt[0 if which == 'fwd' else 1] != kind:
                continue
            for form in H.case_forms(case):
                for field in H.Form._fields:
                    seen[field].add(getattr(form, field))
        want = dict(act=set(H.ACTS), bias=set(H.BIASES), labels=set(H.LABELS), grads=set(H.GRADS), p=set(H.PS), kind=set(H.KINDS))
        assert seen == want, (which, kind, seen)
    for case in H.CASES:                               # the shapes the ABI accepts and nothing else exercised
        assert all(f.labels != 'two' for f in H.case_forms(case)) == (case[1] < 3)
    assert {c[0] for c in H.CASES} == {1, 2, 3} and any(c[4] == 1 for c in H.CASES) and any(c[4] == c[0] * c[2] for c in H.CASES)


def test_head_hip_still_dispatches_as_route_restates():
    """A change of the limit or of either LDS-size formula in csrc/head.hip fails here instead of silently moving the boundaries away
    from the cases; the lines are the ones the docstring of head_ref.route() names."""
    with open(HEAD_HIP) as f:
        lines = f.read().splitlines()
    at = lambda n: ' '.join(lines[n - 1].split())
    assert at(153) == ('static inline size_t head_fwd_lds_floats(int B, int K, int H1) '
                       '{ return (size_t)K * (H1 + 1) + (size_t)B * K + (size_t)B * H1; }')
    assert at(154) == ('static inline size_t head_bwd_lds_floats(int B, int K, int H1, int L) '
                       '{ return (size_t)B * K + (size_t)B * H1 + (size_t)B * L; }')
    assert at(292) == 'const size_t lds = sizeof(float) * head_fwd_lds_floats(B, nseg * D, H1);'
    assert at(293) == 'if (lds <= 150 * 1024 && L <= nseg * D) {'
    assert at(316) == 'const size_t lds = sizeof(float) * head_bwd_lds_floats(B, nseg * D, H1, L);'
    assert at(317) == 'if (lds <= 150 * 1024) {'
    assert H.LDS_LIMIT == 150 * 1024
    text = '\n'.join(lines)
    assert text.count('k_head_fwd_simple') == 2 and text.count('k_head_bwd_simple') == 2      # one definition, one launch each


# ---------------------------------------------------------------------------------------------- inputs
@pytest.mark.parametrize('case', list(H.CASES))
def test_inputs_keep_their_distance_from_the_kink(case):
    for kind in H.KINDS:
        c = H.inputs(case, kind)
        assert H.margin(c) >= H.MARGIN, (case, kind, H.margin(c))
        assert len(c.xs) == case[0] and all(x.shape == (case[1], case[2]) and x.dtype == torch.float32 for x in c.xs)
    r = H.reference_of(case, H.Form(1, True, 'valid', 'both', 0.0, 'normal'))
    assert 0.05 <= float(r.z.abs().mean()) <= 5.0 and float(r.logits.abs().max()) <= 10.0
    big = H.reference_of(case, H.Form(1, True, 'valid', 'both', 0.0, 'large'))
    top = float(big.logits.abs().max())
    assert top == 0.0 or 99.0 <= top <= 101.0, (case, top)


def test_large_logits_overflow_float32_without_the_max_subtraction():
    big = H.reference_of(H.BASE, H.Form(1, True, 'valid', 'both', 0.0, 'large'))
    assert bool(torch.isinf(torch.exp(big.logits.float())).any())
    # the smallest legal call has one class: its loss is exactly 0
    assert float(H.compute(H.arguments((1, 1, 1, 1, 1), H.ROTATION[0])).loss) == 0.0


# ---------------------------------------------------------------------------------------------- the float32 twin and its mutants
@pytest.mark.parametrize('case', list(H.CASES))
def test_twin(case):
    worst = H.Excess()
    for form in H.case_forms(case):
        a = H.arguments(case, form)
        for name, e in judged(a, H.reference_of(case, form), H.twin(a)).items():
            worst.add(name, e)
    print('HEAD twin %r: %s' % (case, worst.line()))
    for name, e in worst.items():
        limit = E32.get((case, name), 0.25)
        assert e <= limit, '%r %s: e32 = %.3g above %.3g' % (case, name, e, limit)


# mutant -> the (case, form) on which it has to show
MUTANT_CASES = {
    'mean_over_B': (H.BASE, H.Form(1, True, 'two', 'both', 0.2, 'normal')),
    'no_keep_bwd': (H.BASE, H.Form(2, True, 'valid', 'both', 0.5, 'normal')),
    'elu_at_h': ((3, 165, 60, 50, 3), H.Form(2, False, 'two', 'dloss', 0.5, 'normal')),
    'leaky_slope': ((3, 128, 60, 50, 3), H.Form(3, False, 'valid', 'ext', 0.0, 'normal')),
    'b2_dropped': ((2, 33, 7, 13, 4), H.Form(1, True, 'valid', 'both', 0.2, 'normal')),
    'segments_swapped': (H.BASE, H.Form(0, False, 'null', 'ext', 0.2, 'normal')),
    'dx_shifted': ((3, 41, 300, 50, 3), H.Form(1, True, 'valid', 'both', 0.2, 'normal')),
    'no_max': (H.BASE, H.Form(1, True, 'valid', 'both', 0.0, 'large')),
    'no_ext': (H.BASE, H.Form(3, True, 'ignored', 'both', 0.0, 'normal')),
    'dropout_index': (H.BASE, H.Form(1, True, 'valid', 'both', 0.2, 'normal')),
}


def test_the_mutant_list_is_the_one_of_head_ref():
    assert set(MUTANT_CASES) == set(H.MUTANTS)


@pytest.mark.parametrize('mutant', H.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    """The unmutated twin passes the case; the mutant exceeds the bound of at least one output by a factor of 10 or more."""
    case, form = MUTANT_CASES[mutant]
    assert form in H.case_forms(case)
    a = H.arguments(case, form)
    ref = H.reference_of(case, form)
    clean = judged(a, ref, H.twin(a))
    assert all(e <= bound(case, name) for name, e in clean.items()), clean.line()
    ex = judged(a, ref, H.twin(a, mutant))
    print('HEAD mutant %s: %s' % (mutant, ex.line()))
    assert any(e >= 10.0 * bound(case, name) for name, e in ex.items()), (mutant, ex.line())


# ---------------------------------------------------------------------------------------------- the dropout plane
@pytest.mark.parametrize('p', [0.2, 0.5])
def test_keep_plane_properties(p):
    B, H1 = 165, 50
    n = B * H1
    scale = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32)))
    planes = [H.keep_plane(seed, B, H1, p) for seed in H.SEEDS + (H.SEED,)]
    for k in planes:
        assert k.dtype == torch.float32 and k.shape == (B, H1)
        assert set(k.unique().tolist()) == {0.0, scale}
        kept = float((k != 0).sum())
        assert abs(kept - n * (1 - p)) <= 4.0 * (n * p * (1 - p)) ** 0.5, (kept, n * (1 - p))
    for i in range(len(planes)):
        for j in range(i):
            assert not torch.equal(planes[i], planes[j])
    # element i = b * H1 + j draws from the counter i alone: a smaller batch is a prefix, whatever the launch shape
    assert torch.equal(H.keep_plane(H.SEED, 127, H1, p), planes[-1][:127])
    assert torch.equal(H.keep_plane(H.SEED, B, H1, 0.0), torch.ones(B, H1))
    # the first draw of seed 0, written out: splitmix64(0x9E3779B97F4A7C15) = 0xE220A8397B1DCDAF -> u = 0xE220A8 / 2^24 = 0.883
    assert float(H.keep_plane(0, 1, 1, 0.88)) != 0.0 and float(H.keep_plane(0, 1, 1, 0.89)) == 0.0
