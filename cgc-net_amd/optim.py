"""The reference's optimisers (common/utils.py:119-127, init_optim: Adam, SGD and RMSprop) without torch's per-step bookkeeping.

``torch.optim.Adam(fused=True).step()`` regroups ~100 parameters by device and dtype and rebuilds five lists on every call
(~0.25 ms of host time; at 4 graphs per GPU the GPU waits for it between the end of backward and the update); SGD and RMSprop do the
same.  Each class here has three levels:

* torch's own ``step()`` on the first step (it creates the state) and whenever something below does not apply;
* the lists do not change from step to step, so they are built once; ``step`` then calls the kernels torch's own ``step`` ends in,
  with the same arguments: ``torch._fused_adam_`` / ``torch._fused_sgd_`` / RMSprop's foreach sequence (any model);
* ``Adam(params, model=encoder)`` (likewise ``SGD``, ``RMSprop``): when the step sequencer produced the gradients
  (network.SoftPoolingGcnEncoder on its default path), every parameter's gradient sits at a fixed offset of one of four flat
  buffers (native._register_flat), and the whole update is ONE launch of the library's ``cgc_adam_step`` / ``cgc_sgd_step`` /
  ``cgc_rmsprop_step`` over a segment table built once: no lists, no step-counter kernel, no per-tensor metadata.  The arithmetic
  is that of the level above, bit for bit (tests/test_native_gpu.py, tests/test_optim_gpu.py).  Anything unexpected -- a gradient
  that is not where the sequencer leaves it (accumulation over several backward passes, a parameter trained through the
  per-operator path), parameters moved, a parameter without a gradient, AMSGrad / nesterov / centred, a closure, a tensor LR,
  several parameter groups, ... -- falls back to a level above for that step.

State, ``state_dict`` and LR schedulers are torch's (the per-parameter ``step`` tensors are brought up to date before anything reads
them), so checkpoints move freely between these classes and torch's.
"""
import ctypes as C

import torch


class _OneLaunch:
    """What the three optimisers share: cached lists, the segment table of the one-launch path, its readiness checks, grad_mul on
    torch's path and the invalidation on load.  Mixed in before the torch class (``class Adam(_OneLaunch, torch.optim.Adam)``); a
    rule supplies the state keys of the table's two columns, the flags that send a step to torch, and its two update calls."""
    _FALLBACK = ()              # group options under which every step is torch's own
    _STEPS = False              # the rule keeps per-parameter 'step' tensors

    def _setup(self, model, grad_mul):
        self._lists = None
        self._model = model
        self._table = None          # (segs, blocks, nblocks, sentinels, device, state keys) of the one-launch path
        self._ptrs = None           # parameter addresses the table was built for
        self._t = None              # step count of the one-launch path not yet in torch's step tensors (None: they are current)
        self._uneven = False        # (Adam) per-parameter step counts differ: the one-launch kernel (one count for all) is not used
        # every gradient is multiplied by grad_mul inside the update (p.grad itself is left as it is).  For callers that keep SUMMED
        # gradients and want the mean taken here; parallel.DataParallel does NOT use it -- it hands over averaged gradients
        self.grad_mul = grad_mul

    def _state_keys(self, g):
        """State keys of the table's columns m and v (None: a NULL column)."""
        raise NotImplementedError

    def _has_state(self, p, keys):
        st = self.state.get(p, {})          # (.get: self.state is a defaultdict, and a rule without state must not grow entries)
        return all(k is None or st.get(k) is not None for k in keys)

    def _sptr(self, p, k):
        return self.state[p][k].data_ptr() if k is not None else 0

    # ---- torch's kernels on cached lists
    def _cache(self):
        g = self.param_groups[0]
        keys = self._state_keys(g)
        ps = [p for p in g['params'] if p.grad is not None]
        if not ps or not all(self._has_state(p, keys) for p in ps) or len({(p.device, p.dtype) for p in ps}) != 1:
            return None
        st = [self.state.get(p, {}) for p in ps]
        return (ps, [s[keys[0]] for s in st] if keys[0] else None, [s[keys[1]] for s in st] if keys[1] else None,
                [s['step'] for s in st] if self._STEPS else None, len(g['params']))

    # ---- the library's one-launch kernel on the sequencer's flat gradient buffers
    def _build_table(self):
        m = self._model
        index = getattr(m, '_flat_index', None)
        if not index or any(s not in (0, 1, 2, 3) for s in index):
            return False                  # (False: this model's gradients do not come out of the sequencer -- do not try again)
        where = {}
        for slot, items in index.items():
            for p, off in items:
                where[id(p)] = (slot, off)
        ps = self.param_groups[0]['params']
        keys = self._state_keys(self.param_groups[0])
        if any(id(p) not in where or p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or not self._has_state(p, keys)
               for p in ps):
            return False
        dev = ps[0].device
        segs, blocks, sentinels, seen = [], [], {}, set()
        for i, p in enumerate(ps):
            slot, off = where[id(p)]
            segs += [p.data_ptr(), self._sptr(p, keys[0]), self._sptr(p, keys[1]), off, p.numel(), slot]
            blocks += [(i, c) for c in range(-(-p.numel() // 1024))]
            if slot not in seen:
                seen.add(slot)
                sentinels[slot] = (p, off, p.data_ptr(), self._sptr(p, keys[0]))
        self._ptrs = [p.data_ptr() for p in ps]
        seg_t = torch.tensor(segs, dtype=torch.int64).view(-1, 6)
        packed = torch.zeros(len(ps), 6, dtype=torch.int64)        # cgc_adam_seg: 5 x 8 bytes + two int32
        packed[:, :5] = seg_t[:, :5]
        packed[:, 5] = seg_t[:, 5]                                 # slot in the low half (little endian), reserved = 0
        blk = torch.tensor(blocks, dtype=torch.int32).view(-1, 2)
        return (packed.to(dev), blk.to(dev), blk.shape[0], sentinels, dev, keys)

    def _fast_ready(self):
        if not self._table:
            return False
        flat = getattr(self._model, '_flat_grads', None)
        if not flat or self._table[4].index != torch.cuda.current_device():
            return False
        # torch's optimisers skip a parameter without a gradient (frozen after the first step: requires_grad = False + zero_grad());
        # the sequencer still writes that parameter's slice of the flat buffer, so the one-launch kernel must not run then
        if any(p.grad is None for p in self.param_groups[0]['params']):
            return False
        # the table holds raw addresses: every parameter must still live where it did (model.to(), p.data = ..., assign=True loads),
        # and its columns must still be the state the rule reads now (a momentum switched on or off)
        if ([p.data_ptr() for p in self.param_groups[0]['params']] != self._ptrs
                or self._table[5] != self._state_keys(self.param_groups[0])):
            self._table = None               # rebuilt by the next step()
            return False
        key = self._table[5][0]
        for slot, (p, off, pptr, mptr) in self._table[3].items():
            g, f = p.grad, flat.get(slot)
            if g is None or f is None or g.data_ptr() != f.data_ptr() + 4 * off or self._sptr(p, key) != mptr:
                return False
        return True

    def _torch_step(self, closure=None):
        return super().step(closure)

    def _scaled_step(self, closure=None):
        """torch's own step with grad_mul applied (the one-launch kernel applies it itself).  The caller's p.grad tensors are left
        untouched: scaled copies stand in for them during the call."""
        if self.grad_mul == 1.0 or closure is not None:
            return self._torch_step(closure)
        ps = [p for gr in self.param_groups for p in gr['params'] if p.grad is not None]
        keep = [p.grad for p in ps]
        for p, g in zip(ps, torch._foreach_mul(keep, self.grad_mul) if keep else []):
            p.grad = g
        try:
            return self._torch_step()
        finally:
            for p, g in zip(ps, keep):
                p.grad = g

    def _flush_steps(self):
        """Bring torch's per-parameter ``step`` tensors up to date with the one-launch path's counter."""
        self._t = None

    def _fast_allowed(self, g):
        return True

    def state_dict(self):
        self._flush_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self._t, self._table, self._lists, self._uneven = None, None, None, False
        return super().load_state_dict(state_dict)

    @torch.no_grad()
    def step(self, closure=None):
        g = self.param_groups[0]
        if (closure is not None or len(self.param_groups) != 1 or any(g.get(f) for f in self._FALLBACK)
                or not isinstance(g['lr'], float)):
            self._flush_steps()
            return self._scaled_step(closure)
        # (a parameter that gets its first gradient on a later step, or loses it: the cached lists are rebuilt)
        if self._lists is not None and (self._lists[4] != len(g['params'])
                                        or sum(p.grad is not None for p in g['params']) != len(self._lists[0])):
            self._lists = None
        if self._lists is None:
            self._flush_steps()
            out = self._scaled_step()                 # torch's own path creates the state on the first step
            self._lists = self._cache()
            self._uneven = False                      # re-examined on the next step: uneven step counts can be transient
            if self._model is not None and self._lists is not None and self._table is None:
                self._table = self._build_table()
            return out
        if self._model is not None and self._table is None and self._lists is not None:
            self._table = self._build_table()          # (invalidated: parameters were moved)
        if self._model is not None and self._fast_ready() and self._fast_allowed(g):
            from . import kernels
            flat = self._model._flat_grads
            segs, blocks, nblocks = self._table[:3]
            K = kernels.get()
            bases = (C.c_void_p * 4)(*[flat[s].data_ptr() if s in flat else None for s in range(4)])
            name, rc = self._launch(K.lib, (C.c_void_p(segs.data_ptr()), C.c_void_p(blocks.data_ptr()), nblocks, bases), g, K._stream())
            if rc != 0:
                raise RuntimeError('%s failed with code %d' % (name, rc))
            return None
        self._flush_steps()
        ps, m, v, steps, _ = self._lists
        grads = [p.grad for p in ps]
        if any(x is None for x in grads):
            self._lists = None
            return self._scaled_step()
        if self.grad_mul != 1.0:
            grads = list(torch._foreach_mul(grads, self.grad_mul))
        self._list_step(g, ps, grads, m, v, steps)
        return None


class Adam(_OneLaunch, torch.optim.Adam):
    _FALLBACK = ('amsgrad', 'maximize', 'capturable', 'differentiable')
    _STEPS = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, model=None, grad_mul=1.0):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=True)
        self._setup(model, grad_mul)

    def _state_keys(self, g):
        return ('exp_avg', 'exp_avg_sq')

    def _flush_steps(self):
        # the one-launch path counts for every parameter at once: torch's step tensors are SET to that count
        if self._t is not None:
            steps = [self.state[p]['step'] for p in self.param_groups[0]['params'] if 'step' in self.state[p]]
            if steps:
                torch._foreach_zero_(steps)
                torch._foreach_add_(steps, float(self._t))
            self._t = None

    def _fast_allowed(self, g):
        # (one device read, the first time only)  The kernel takes ONE step count for all parameters: if they differ -- a parameter
        # sat out some steps without a gradient -- the bias corrections differ per parameter and torch's kernel stays
        if self._uneven:
            return False
        if self._t is None:
            st = torch.stack([self.state[p]['step'] for p in g['params']])
            lo, hi = float(st.min()), float(st.max())
            if lo != hi:
                self._uneven = True
                return False
            self._t = int(hi)
        return True

    def _launch(self, lib, tables, g, stream):
        self._t += 1
        return 'cgc_adam_step', lib.cgc_adam_step(*tables, g['lr'], g['betas'][0], g['betas'][1], g['weight_decay'], g['eps'],
                                                  float(self._t), float(self.grad_mul), stream)

    def _list_step(self, g, ps, grads, m, v, steps):
        torch._foreach_add_(steps, 1)
        torch._fused_adam_(ps, grads, m, v, [], steps, amsgrad=False, lr=g['lr'], beta1=g['betas'][0], beta2=g['betas'][1],
                           weight_decay=g['weight_decay'], eps=g['eps'], maximize=False, grad_scale=None, found_inf=None)


class SGD(_OneLaunch, torch.optim.SGD):
    """torch.optim.SGD(fused=True); table columns: m = momentum_buffer (NULL without momentum).  A parameter whose buffer does not
    exist yet (its first step, or a loaded state without one) leaves that step to torch, which copies the gradient into it."""
    _FALLBACK = ('nesterov', 'maximize', 'capturable', 'differentiable')

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, model=None, grad_mul=1.0):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         fused=True)
        self._setup(model, grad_mul)

    def _state_keys(self, g):
        return ('momentum_buffer' if g['momentum'] != 0 else None, None)

    def _torch_step(self, closure=None):
        # torch's fused SGD refuses a step in which some parameters have a momentum buffer and others not yet (a parameter whose
        # first gradient arrives late); torch's foreach implementation takes that step, as torch.optim.SGD() would
        mixed = []
        for gr in self.param_groups:
            if gr['fused'] and gr['momentum'] != 0:
                has = [self.state[p].get('momentum_buffer') is not None for p in gr['params'] if p.grad is not None]
                if any(has) and not all(has):
                    mixed.append(gr)
        for gr in mixed:
            gr['fused'] = False
        try:
            return super()._torch_step(closure)
        finally:
            for gr in mixed:
                gr['fused'] = True

    def _launch(self, lib, tables, g, stream):
        return 'cgc_sgd_step', lib.cgc_sgd_step(*tables, g['lr'], g['momentum'], g['dampening'], g['weight_decay'],
                                                float(self.grad_mul), stream)

    def _list_step(self, g, ps, grads, m, v, steps):
        torch._fused_sgd_(ps, grads, m if g['momentum'] != 0 else [], weight_decay=g['weight_decay'], momentum=g['momentum'],
                          lr=g['lr'], dampening=g['dampening'], nesterov=False, maximize=False, is_first_step=False,
                          grad_scale=None, found_inf=None)


class RMSprop(_OneLaunch, torch.optim.RMSprop):
    """torch.optim.RMSprop(foreach=True), not centred; table columns: m = square_avg, v = momentum_buffer (NULL without momentum).
    The update does not read ``step``: the one-launch path counts on the host, and the count is ADDED to every parameter's step
    tensor before anything reads them (per-parameter counts may differ)."""
    _FALLBACK = ('centered', 'maximize', 'capturable', 'differentiable')
    _STEPS = True

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False, model=None,
                 grad_mul=1.0):
        super().__init__(params, lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=centered,
                         foreach=True)
        self._setup(model, grad_mul)

    def _state_keys(self, g):
        return ('square_avg', 'momentum_buffer' if g['momentum'] > 0 else None)

    def _flush_steps(self):
        if self._t is not None:
            steps = [self.state[p]['step'] for p in self.param_groups[0]['params'] if 'step' in self.state.get(p, {})]
            if steps:
                torch._foreach_add_(steps, float(self._t))
            self._t = None

    def _launch(self, lib, tables, g, stream):
        self._t = (self._t or 0) + 1
        return 'cgc_rmsprop_step', lib.cgc_rmsprop_step(*tables, g['lr'], g['alpha'], g['eps'], g['weight_decay'], g['momentum'],
                                                        float(self.grad_mul), stream)

    def _list_step(self, g, ps, grads, m, v, steps):
        # torch/optim/rmsprop.py _multi_tensor_rmsprop, not centred, not maximised: the same foreach calls with the same arguments
        lr, alpha, eps, wd, momentum = g['lr'], g['alpha'], g['eps'], g['weight_decay'], g['momentum']
        torch._foreach_add_(steps, 1.0)
        if wd != 0:
            grads = torch._foreach_add(grads, ps, alpha=wd)
        torch._foreach_mul_(m, alpha)
        torch._foreach_addcmul_(m, grads, grads, value=1 - alpha)
        avg = torch._foreach_sqrt(m)
        torch._foreach_add_(avg, eps)
        if momentum > 0:
            torch._foreach_mul_(v, momentum)
            torch._foreach_addcdiv_(v, grads, avg)
            torch._foreach_add_(ps, v, alpha=-lr)
        else:
            torch._foreach_addcdiv_(ps, grads, avg, value=-lr)


def init_optim(optim, params, lr, weight_decay, model=None):
    """common/utils.py:119-127 with this module's classes: ``model`` (the encoder) enables the one-launch update."""
    if optim == 'adam':
        return Adam(params, lr=lr, weight_decay=weight_decay, model=model)
    elif optim == 'sgd':
        return SGD(params, lr=lr, momentum=0.9, weight_decay=weight_decay, model=model)
    elif optim == 'rmsprop':
        return RMSprop(params, lr=lr, momentum=0.9, weight_decay=weight_decay, model=model)
    else:
        raise KeyError("Unsupported optim: {}".format(optim))
