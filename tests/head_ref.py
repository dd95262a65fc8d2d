"""Float64 reference of the classification head (csrc/head.hip: cat(readouts) -> Linear -> act -> Dropout -> Linear -> mean
cross-entropy, and its backward) for tests/test_head_ref_cpu.py and tests/test_head_fp64_gpu.py, written from the contract in head.hip
and the layers it cites, forward and backward spelled out (the CPU file holds it to autograd through nn.Linear / F.cross_entropy).

Beside each value the reference returns its ``terms``: the same expression with every operand replaced by its magnitude -- leaves are
|x|, |W|, |b|, softmax probabilities and one-hots as they are, every activation counts as 1-Lipschitz:
terms(z) = |b1| + |W1||x|, terms(h) = keep * terms(z), terms(logits) = |b2| + |W2| terms(h), terms(per-sample loss) = max_l
terms(logits) + log L + terms(logit_y) (|logsumexp| <= max|logit| + log L), terms(dl) = |g| (p + onehot) + |dlogits_ext|, and on
through dW2 = dl^T h, dh = dl W2, dz = dh keep act'(z), dW1 = dz^T x, dx = dz W1.

Label semantics are head.hip's: -100 is skipped and the mean runs over the rest; any other label outside [0, L) makes the loss NaN
and, where a loss gradient is asked for, the gradient of every sample that is not skipped -- and with it every parameter gradient.
All labels -100: the loss is 0/0 = NaN and every gradient is exactly zero, which is what F.cross_entropy returns in float64 on the
CPU for that input (tests/test_head_ref_cpu.py::test_all_ignored_labels_are_what_cross_entropy_returns).

The same code in float32 is the twin that measures the yardstick on the CPU; ``mutant`` turns it into one of MUTANTS, each a single
subtle error the judge has to reject.  Also here: the dropout plane restated with Python integers (``keep_plane``), the host dispatch
restated (``route``), the cases and argument forms, the inputs (repaired so that no pre-activation lies within MARGIN of the kink),
the direct calls of cgc_head_fwd / cgc_head_bwd into canary-guarded buffers of exactly the documented sizes, and the judges."""
import collections
import ctypes
import functools
import math

import numpy as np
import torch

# the project's yardsticks and placement, shared with the row and SAGE tests (re-exported for the two test files)
from rowops_ref import ATOL_SUM, CANARY, MARGIN, RTOL_SUM, Bag, Excess, Place, cached, excess_point, excess_sum  # noqa: F401

IGNORE = -100
LDS_LIMIT = 150 * 1024
DLOSS = 0.75                              # exact in float32
SEED = 0xC0FFEE1234567891                 # above 2^63: a seed truncated or sign-mangled on its way to the kernel changes the plane
SEEDS = (0, 1, 2 ** 63, 2 ** 64 - 1)

# (nseg, B, D, H1, L) -> the kernels cgc_head_fwd / cgc_head_bwd launch there, as the issue's table has them; route() must agree
CASES = collections.OrderedDict([
    ((3, 37, 60, 50, 3), ('lds', 'lds')),             # base: B * H1 > 1024, the thread-stride loops wrap
    ((3, 127, 60, 50, 3), ('lds', 'lds')),            # forward boundary at the network's widths
    ((3, 128, 60, 50, 3), ('simple', 'lds')),
    ((3, 164, 60, 50, 3), ('simple', 'lds')),         # backward boundary
    ((3, 165, 60, 50, 3), ('simple', 'simple')),
    ((3, 1, 64, 196, 5), ('lds', 'lds')),             # W1 alone fills the LDS at B = 1
    ((3, 1, 64, 197, 5), ('simple', 'lds')),
    ((3, 40, 300, 50, 3), ('simple', 'lds')),         # backward boundary at a small B
    ((3, 41, 300, 50, 3), ('simple', 'simple')),
    ((1, 4, 8, 6, 8), ('lds', 'lds')),                # L == K: the logits fill x's LDS exactly
    ((1, 4, 8, 6, 9), ('simple', 'lds')),             # L > K
    ((2, 33, 7, 13, 4), ('lds', 'lds')),              # two segments, odd extents
    ((1, 1, 1, 1, 1), ('lds', 'lds')),                # smallest legal call; the loss is exactly 0
])
BASE = (3, 37, 60, 50, 3)


def route(nseg, B, D, H1, L):
    """-> (fwd, bwd), each 'lds' or 'simple': the host conditions of csrc/head.hip -- head_fwd_lds_floats and head_bwd_lds_floats
    (lines 153-154), `lds <= 150 * 1024 && L <= nseg * D` of cgc_head_fwd (line 293), `lds <= 150 * 1024` of cgc_head_bwd (line 317)."""
    K = nseg * D
    fwd_floats = K * (H1 + 1) + B * K + B * H1
    bwd_floats = B * K + B * H1 + B * L
    return ('lds' if 4 * fwd_floats <= LDS_LIMIT and L <= K else 'simple', 'lds' if 4 * bwd_floats <= LDS_LIMIT else 'simple')


# ------------------------------------------------------------------------------------------------ argument forms
Form = collections.namedtuple('Form', 'act bias labels grads p kind')
ACTS = (0, 1, 2, 3)
BIASES = (True, False)
LABELS = ('valid', 'two', 'ignored', 'null')          # all valid, two -100, all -100, y NULL
GRADS = ('dloss', 'ext', 'both', 'neither')
PS = (0.0, 0.2, 0.5)
KINDS = ('normal', 'large')                           # 'large': logits of magnitude ~100, see inputs()

# what every case but the base case runs: each value of each axis at least once
ROTATION = (
    Form(1, True, 'valid', 'both', 0.2, 'normal'),
    Form(2, False, 'two', 'dloss', 0.5, 'normal'),
    Form(3, True, 'ignored', 'both', 0.0, 'normal'),
    Form(0, False, 'null', 'ext', 0.2, 'normal'),
    Form(2, True, 'valid', 'neither', 0.5, 'normal'),
    Form(3, False, 'valid', 'ext', 0.0, 'normal'),
    Form(0, True, 'two', 'dloss', 0.0, 'normal'),
    Form(1, True, 'valid', 'both', 0.0, 'large'),
)


def base_forms(act):
    """The full cross of the base case for one activation (the GPU file runs one test per activation), plus the large logits."""
    out = [Form(act, bias, lab, gr, p, 'normal') for bias in BIASES for lab in LABELS for gr in GRADS for p in PS]
    return out + [Form(act, True, 'valid', 'both', 0.0, 'large')]


def case_forms(case):
    """The forms a case runs.  With fewer than 3 samples 'two -100' has no two samples to skip beside a valid one: those cases run
    the form with every label valid instead."""
    if case == BASE:
        return [f for act in ACTS for f in base_forms(act)]
    if case[1] >= 3:
        return list(ROTATION)
    return [f._replace(labels='valid') if f.labels == 'two' else f for f in ROTATION]


# ------------------------------------------------------------------------------------------------ the dropout plane
@functools.lru_cache(maxsize=None)
def _keep_plane(seed, B, H1, p):
    if p <= 0:
        return np.ones((B, H1), dtype=np.float32)
    M = (1 << 64) - 1
    p32 = np.float32(p)
    scale = np.float32(1) / (np.float32(1) - p32)
    out = np.empty(B * H1, dtype=np.float32)
    for i in range(B * H1):
        z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        u = np.float32(z >> 40) * np.float32(1.0 / 16777216.0)           # a 24-bit integer times 2^-24: exact
        out[i] = np.float32(0) if u < p32 else scale
    return out.reshape(B, H1)


def keep_plane(seed, B, H1, p):
    """head_keep of csrc/head.hip for element i = b * H1 + j, restated with Python integers and numpy float32 -> float32 [B, H1]."""
    return torch.from_numpy(_keep_plane(int(seed), int(B), int(H1), float(p)).copy())


# ------------------------------------------------------------------------------------------------ the operator
MUTANTS = ('mean_over_B', 'no_keep_bwd', 'elu_at_h', 'leaky_slope', 'b2_dropped', 'segments_swapped', 'dx_shifted', 'no_max',
           'no_ext', 'dropout_index')


def _act(z, act, leaky):
    if act == 0:
        return z
    if act == 1:
        return torch.relu(z)
    if act == 2:
        return torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0.0)))
    if act == 3:
        return torch.where(z > 0, z, leaky * z)
    raise ValueError(act)


def _dact(z, act, leaky):
    one = torch.ones_like(z)
    if act == 0:
        return one
    if act == 1:
        return (z > 0).to(z.dtype)
    if act == 2:
        return torch.where(z > 0, one, torch.exp(torch.clamp(z, max=0.0)))
    if act == 3:
        return torch.where(z > 0, one, leaky * one)
    raise ValueError(act)


def reference(xs, W1, b1, W2, b2, y, keep, act, dloss, dlogits_ext, dtype=torch.float64, mutant=None):
    """xs: 1..3 readouts [B, D]; b1, b2, y, dloss (a Python float), dlogits_ext may be None; keep [B, H1] is the dropout keep-scale.
    -> Bag: z, h, logits, per (per-sample loss, 0 at skipped samples), loss, dl, dz, dW1, db1, dW2, db2, dx (list), keep; beside each
    value v its terms t_v.  per, loss and their terms are None without labels."""
    assert mutant is None or mutant in MUTANTS, mutant
    cv = lambda t: None if t is None else t.detach().cpu().to(dtype)
    xs = [cv(x) for x in xs]
    W1, b1, W2, b2, keep, ext = cv(W1), cv(b1), cv(W2), cv(b2), cv(keep), cv(dlogits_ext)
    nseg, (B, D) = len(xs), xs[0].shape
    H1, L = W1.shape[0], W2.shape[0]
    order = [0, 2, 1] if mutant == 'segments_swapped' and nseg == 3 else list(range(nseg))
    x = torch.cat([xs[s] for s in order], 1)
    if mutant == 'dropout_index':                      # element (b, j) takes the draw of index j * B + b
        keep = keep.reshape(H1, B).t().contiguous()
    leaky = 0.1 if mutant == 'leaky_slope' else 0.01
    r = Bag(keep=keep)
    r.z, r.t_z = x @ W1.t(), x.abs() @ W1.abs().t()
    if b1 is not None:
        r.z, r.t_z = r.z + b1, r.t_z + b1.abs()
    r.h, r.t_h = _act(r.z, act, leaky) * keep, keep * r.t_z
    r.logits, r.t_logits = r.h @ W2.t(), r.t_h @ W2.abs().t()
    if b2 is not None:
        r.logits, r.t_logits = (r.logits if mutant == 'b2_dropped' else r.logits + b2), r.t_logits + b2.abs()
    lg = r.logits
    r.per = r.t_per = r.loss = r.t_loss = None
    r.dl, r.t_dl = torch.zeros(B, L, dtype=dtype), torch.zeros(B, L, dtype=dtype)
    if y is not None:
        y = y.detach().cpu().long().reshape(-1)
        ok = (y >= 0) & (y < L)
        skipped = y == IGNORE
        bad = bool((~ok & ~skipped).any())
        count = float(B) if mutant == 'mean_over_B' else float(ok.sum())
        denom = torch.tensor(float('nan') if bad else count, dtype=dtype)
        yi = torch.where(ok, y, torch.zeros_like(y))
        onehot = torch.zeros(B, L, dtype=dtype)
        onehot[torch.arange(B), yi] = 1.0
        onehot = onehot * ok.to(dtype).unsqueeze(1)
        if mutant == 'no_max':
            e = torch.exp(lg)
            s = e.sum(1, keepdim=True)
            lse = torch.log(s[:, 0])
        else:
            m = lg.max(1, keepdim=True).values
            e = torch.exp(lg - m)
            s = e.sum(1, keepdim=True)
            lse = m[:, 0] + torch.log(s[:, 0])
        p = e / s
        zero = torch.zeros(B, dtype=dtype)
        r.per = torch.where(ok, lse - lg.gather(1, yi.unsqueeze(1))[:, 0], zero)
        r.t_per = torch.where(ok, r.t_logits.max(1).values + math.log(L) + r.t_logits.gather(1, yi.unsqueeze(1))[:, 0], zero)
        r.loss, r.t_loss = r.per.sum() / denom, r.t_per.sum() / denom
        if dloss is not None:
            g = torch.tensor(float(np.float32(dloss)), dtype=dtype) / denom
            live = (ok if not bad else ~skipped).unsqueeze(1)          # a corrupt label poisons every sample that is not skipped
            r.dl = torch.where(live, g * (p - onehot), r.dl)
            r.t_dl = torch.where(live, g.abs() * (p + onehot), r.t_dl)
    if ext is not None:
        if mutant != 'no_ext':
            r.dl = r.dl + ext
        r.t_dl = r.t_dl + ext.abs()
    r.dW2, r.t_dW2 = r.dl.t() @ r.h, r.t_dl.t() @ r.t_h
    r.db2, r.t_db2 = r.dl.sum(0), r.t_dl.sum(0)
    dh, t_dh = r.dl @ W2, r.t_dl @ W2.abs()
    r.dz = dh * _dact(r.h if mutant == 'elu_at_h' else r.z, act, leaky)
    if mutant != 'no_keep_bwd':
        r.dz = r.dz * keep
    r.t_dz = t_dh * keep
    r.dW1, r.t_dW1 = r.dz.t() @ x, r.t_dz.t() @ x.abs()
    r.db1, r.t_db1 = r.dz.sum(0), r.t_dz.sum(0)
    dx, t_dx = r.dz @ W1, r.t_dz @ W1.abs()
    r.dx = [dx[:, s * D:(s + 1) * D] for s in range(nseg)]
    r.t_dx = [t_dx[:, s * D:(s + 1) * D] for s in range(nseg)]
    if mutant == 'dx_shifted':                         # segment s lands in the buffer of segment s - 1; the last buffer stays as it was
        r.dx = r.dx[1:] + [torch.full((B, D), CANARY, dtype=dtype)]
    return r


# ------------------------------------------------------------------------------------------------ inputs
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _preacts(x, W1, b1):
    z0 = x.double() @ W1.double().t()
    return z0, z0 + b1.double()


def _repair(x, W1, b1):
    """Moves x[b] along W1[j] for every (b, j) whose pre-activation, with or without b1, lies within 2 * MARGIN of zero, until none is
    left: a step of delta along W1[j] / |W1[j]|^2 moves z[b, j] by delta and its neighbours by a few percent of that."""
    W = W1.double()
    x = x.clone()
    for _ in range(2000):
        z0, z1 = _preacts(x, W1, b1)
        off = torch.nonzero((z0.abs() < 2 * MARGIN) | (z1.abs() < 2 * MARGIN))
        if off.shape[0] == 0:
            return x
        b, j = int(off[0, 0]), int(off[0, 1])
        for step in (1, -1, 2, -2, 3, -3, 4, -4, 6, -6, 8, -8):
            delta = step * 4 * MARGIN
            if abs(float(z0[b, j]) + delta) >= 3 * MARGIN and abs(float(z1[b, j]) + delta) >= 3 * MARGIN:
                break
        x[b] = (x[b].double() + delta * W[j] / float(W[j] @ W[j])).float()
    raise AssertionError('the pre-activations could not be moved off the kink')


@functools.lru_cache(maxsize=None)
def inputs(case, kind='normal'):
    """Seeded by the case.  x ~ N(0, 1), W1 ~ N(0, 1/K), W2 ~ N(0, 1/H1), biases and dlogits_ext ~ 0.1 N(0, 1): z and the logits are
    O(1).  x is repaired so that every |z|, with and without b1, is at least MARGIN.  kind 'large' scales W2 and b2 so that the
    largest |logit| (ReLU, no dropout) is 100: expf of such a logit overflows float32 (e^88.8 > 3.4e38; e^60 = 1.1e26 would not),
    so a softmax without the max subtraction gives inf and NaN there."""
    nseg, B, D, H1, L = case
    K = nseg * D
    rs = np.random.RandomState(list(case))
    c = Bag(case=case, kind=kind, nseg=nseg, B=B, D=D, H1=H1, L=L, K=K)
    x = _f32(rs.standard_normal((B, K)))
    c.W1 = _f32(rs.standard_normal((H1, K)) / math.sqrt(K))
    c.b1 = _f32(0.1 * rs.standard_normal(H1))
    c.W2 = _f32(rs.standard_normal((L, H1)) / math.sqrt(H1))
    c.b2 = _f32(0.1 * rs.standard_normal(L))
    c.y = torch.from_numpy(rs.randint(0, L, size=B).astype(np.int64))
    c.ext = _f32(0.1 * rs.standard_normal((B, L)))
    x = _repair(x, c.W1, c.b1)
    c.xs = [x[:, s * D:(s + 1) * D].contiguous() for s in range(nseg)]
    if kind == 'large':
        top = float(reference(c.xs, c.W1, c.b1, c.W2, c.b2, None, torch.ones(B, H1), 1, None, None).logits.abs().max())
        scale = np.float32(100.0 / top)
        c.W2, c.b2 = c.W2 * scale, c.b2 * scale
    return c


def margin(c):
    """Smallest |pre-activation| of a case's inputs, with and without the bias, in float64."""
    z0, z1 = _preacts(torch.cat(c.xs, 1), c.W1, c.b1)
    return min(float(z0.abs().min()), float(z1.abs().min()))


def labels_of(c, form):
    if form.labels == 'null':
        return None
    y = c.y.clone()
    if form.labels == 'two':
        assert c.B >= 3
        y[0] = y[c.B // 2] = IGNORE
    elif form.labels == 'ignored':
        y[:] = IGNORE
    return y


def arguments(case, form, seed=SEED):
    """The operands of one call: the case's inputs in the given form."""
    c = inputs(case, form.kind)
    return Bag(case=case, form=form, seed=seed, nseg=c.nseg, B=c.B, D=c.D, H1=c.H1, L=c.L, K=c.K, xs=c.xs, W1=c.W1, W2=c.W2,
               b1=c.b1 if form.bias else None, b2=c.b2 if form.bias else None, y=labels_of(c, form), act=form.act, p=form.p,
               keep=keep_plane(seed, c.B, c.H1, form.p), dloss=DLOSS if form.grads in ('dloss', 'both') else None,
               ext=c.ext if form.grads in ('ext', 'both') else None)


def compute(a, dtype=torch.float64, mutant=None):
    return reference(a.xs, a.W1, a.b1, a.W2, a.b2, a.y, a.keep, a.act, a.dloss, a.ext, dtype=dtype, mutant=mutant)


def reference_of(case, form, seed=SEED):
    """The float64 reference of a call, computed once per module run."""
    return cached(('head', case, form, seed), case[1], case[0] * case[2], lambda: compute(arguments(case, form, seed)))


def twin(a, mutant=None):
    """The float32 twin's outputs in the layout of run_forward + run_backward; outputs the kernels would leave alone hold CANARY."""
    r = compute(a, torch.float32, mutant)
    o = dict(z=r.z, keep=r.keep, h=r.h, logits=r.logits, dW1=r.dW1, db1=r.db1, dW2=r.dW2, db2=r.db2, dx=r.dx, dl=r.dl, dz=r.dz)
    o['per'] = r.per if r.per is not None else torch.full((a.B,), CANARY)
    o['loss'] = r.loss.reshape(1) if r.loss is not None else torch.full((1,), CANARY)
    return o


# ------------------------------------------------------------------------------------------------ the direct calls
def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def run_forward(k, P, a, dims=None, drop_p=None):
    """cgc_head_fwd on kernels object k into canary-guarded buffers of exactly the documented sizes: ws = 3*B*H1 + B floats (z | keep |
    h | per-sample losses), logits B*L, loss 1.  ``dims`` = (nseg, B, D, H1, L) and ``drop_p`` override what is passed (the refusal
    tests); the buffers keep the sizes of the case.  -> dict with rc, the views and the device operands."""
    B, H1, L = a.B, a.H1, a.L
    nseg, Bc, D, H1c, Lc = dims if dims is not None else (a.nseg, B, a.D, H1, L)
    d = Bag(xs=[P.inp(x) for x in a.xs], W1=P.inp(a.W1), b1=P.inp(a.b1), W2=P.inp(a.W2), b2=P.inp(a.b2), y=P.inp(a.y))
    m = B * H1
    ws, logits, loss = P.out(3 * m + B), P.out(B, L), P.out(1)
    rc = k.lib.cgc_head_fwd(_ptrs(d.xs), nseg, Bc, D, H1c, Lc, a.act, _ptr(d.W1), _ptr(d.b1), _ptr(d.W2), _ptr(d.b2), _ptr(d.y),
                            ctypes.c_float(a.p if drop_p is None else drop_p), ctypes.c_uint64(a.seed), _ptr(ws), _ptr(logits),
                            _ptr(loss), k._stream())
    return dict(rc=rc, dev=d, ws=ws, z=ws[:m].view(B, H1), keep=ws[m:2 * m].view(B, H1), h=ws[2 * m:3 * m].view(B, H1),
                per=ws[3 * m:], logits=logits, loss=loss)


def run_backward(k, P, a, f, dims=None):
    """cgc_head_bwd over the workspace and logits of the forward ``f`` (run_forward's dict), as a training step does: scratch = B*L +
    B*H1 floats (dl | dz, written by the simple kernel only), grads = dW1 | db1 | dW2 | db2, one [B, D] buffer per readout."""
    B, H1, L, K = a.B, a.H1, a.L, a.K
    nseg, Bc, D, H1c, Lc = dims if dims is not None else (a.nseg, B, a.D, H1, L)
    d = f['dev']
    dloss = P.inp(torch.tensor([a.dloss], dtype=torch.float32)) if a.dloss is not None else None
    ext = P.inp(a.ext)
    scratch, grads = P.out(B * L + B * H1), P.out(H1 * K + H1 + L * H1 + L)
    dx = [P.out(B, a.D) for _ in range(a.nseg)]
    rc = k.lib.cgc_head_bwd(_ptrs(d.xs), nseg, Bc, D, H1c, Lc, a.act, _ptr(d.W1), _ptr(d.W2), _ptr(d.y), _ptr(f['ws']),
                            _ptr(f['logits']), _ptr(dloss), _ptr(ext), _ptr(scratch), _ptr(grads), _ptrs(dx), k._stream())
    o = dict(rc=rc, hold=(dloss, ext), scratch=scratch, grads=grads, dx=dx)
    at = 0
    for name, shape in (('dW1', (H1, K)), ('db1', (H1,)), ('dW2', (L, H1)), ('db2', (L,))):
        n = int(np.prod(shape))
        o[name] = grads[at:at + n].view(shape)
        at += n
    if route(*a.case)[1] == 'simple':
        o['dl'], o['dz'] = scratch[:B * L].view(B, L), scratch[B * L:].view(B, H1)
    return o


# ------------------------------------------------------------------------------------------------ yardsticks
def excess_terms(a, b, terms):
    """|a-b| <= RTOL_SUM * terms + ATOL_SUM per element (rowops_ref.excess_sum); NaN exactly where the reference is NaN; exactly zero
    where the reference is exactly zero (a dropped unit, a gradient nobody asked for, softmax - onehot at L = 1).  -> the excess."""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    t = terms.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape == t.shape, (a.shape, b.shape, t.shape)
    nan = torch.isnan(b)
    if not bool(torch.isnan(a[nan]).all()) or bool((a[b == 0] != 0).any()):
        return float('inf')
    return excess_sum(a[~nan], b[~nan], t[~nan])


def _exact(a, b):
    return 0.0 if torch.equal(a.detach().cpu().float(), b.detach().cpu().float()) else float('inf')


def judge_forward(a, ref, o, ex):
    """keep exact (and with it h exactly 0 where keep is 0, by excess_terms); z, h, logits, the per-sample losses and the loss by
    their terms; without labels the loss and the per-sample slots must still hold the canary."""
    ex.add('keep', _exact(o['keep'], a.keep))
    ex.add('z', excess_terms(o['z'], ref.z, ref.t_z))
    ex.add('h', excess_terms(o['h'], ref.h, ref.t_h))
    ex.add('logits', excess_terms(o['logits'], ref.logits, ref.t_logits))
    if a.y is None:
        ex.add('untouched', _exact(o['loss'], torch.full((1,), CANARY)))
        ex.add('untouched', _exact(o['per'], torch.full((a.B,), CANARY)))
    else:
        ex.add('per', excess_terms(o['per'], ref.per, ref.t_per))
        ex.add('loss', excess_terms(o['loss'], ref.loss, ref.t_loss))


def judge_backward(a, ref, o, ex):
    for name in ('dW1', 'db1', 'dW2', 'db2'):
        ex.add(name, excess_terms(o[name], getattr(ref, name), getattr(ref, 't_' + name)))
    for s in range(a.nseg):
        ex.add('dx', excess_terms(o['dx'][s], ref.dx[s], ref.t_dx[s]))
    if 'dl' in o:
        ex.add('dl', excess_terms(o['dl'], ref.dl, ref.t_dl))
        ex.add('dz', excess_terms(o['dz'], ref.dz, ref.t_dz))


FAMILIES = {'z/h': ('z', 'h', 'keep'), 'logits and loss': ('logits', 'per', 'loss', 'untouched'),
            'parameter gradients': ('dW1', 'db1', 'dW2', 'db2'), 'dx': ('dx', 'dl', 'dz')}
