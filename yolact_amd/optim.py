"""`SGD` — torch.optim.SGD(lr, momentum, weight_decay) as the reference's train.py:215-216 builds it, with step() as ONE launch of
csrc/sgd.hip per parameter group.

    opt = SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    loss.backward()
    opt.step(loss)              # guarded by isfinite(loss) ON THE DEVICE (train.py:317 reads it on the host), gradients zeroed

The arithmetic is the once-rounded contract of ymi_sgd_step_f32 (include/yolact_amd.h): d = g + wd p, m = mom m + d, p = p - lr m,
each operation rounded to fp32, which numpy restates bit for bit; torch's own kernels contract to FMAs, so these are not its bits.
`param_groups` and the state key `momentum_buffer` are torch's: the reference's set_lr works unchanged and state_dict() loads into
torch.optim.SGD and back.  Dampening and Nesterov are not offered.

The kernel writes through raw pointers, so autograd does not see the update.  After an APPLIED step the version counter of every
updated parameter is bumped (torch.autograd.graph.increment_version): Yolact._param_stamp() changes and the inference plans rebuild.
A step without a guard is bumped at once.  Whether a guarded step was applied is only known on the device, and step() never reads
it: such steps are counted, and settle() — which Yolact._param_stamp() calls through settle_all() — reads the `skipped` counter once
and bumps if any of them was applied.  `skipped` counts steps, whatever the number of parameter groups: the first launch of a step
alone is handed the counter.  A cache keyed on a version counter that must not wait for that (dcn_v2's packed filters, read inside a
differentiable forward) adds guarded_writes(tensor) to its key.
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch
from torch.utils.weak import WeakIdKeyDictionary

from . import _lib as L

_LIVE = weakref.WeakSet()
_guarded_writes = WeakIdKeyDictionary()      # parameter -> how many guarded launches covered it, ever (guarded_writes)
_outstanding = 0            # guarded steps not settled yet, over every SGD: what an inference forward pays to look at is this integer


def settle_all():
    """settle() of every live SGD with guarded steps outstanding (Yolact._param_stamp)."""
    global _outstanding
    if not _outstanding:
        return
    for opt in list(_LIVE):
        if opt._guarded:
            opt.settle()
    _outstanding = sum(opt._guarded for opt in list(_LIVE))      # (an optimiser that died with steps outstanding took them along)


def guarded_writes(t):
    """How many loss-guarded launches have covered the tensor `t` so far.  A cache keyed on t._version adds this to its key: the
    version bump of a guarded step waits for settle(), this count moves with the launch (also for a step that turns out skipped: one
    spurious rebuild), and reading it neither waits for the device nor touches a counter autograd may be holding saved tensors to."""
    return _guarded_writes.get(t, 0) if t is not None else 0


class _Table:
    """The device tables of one parameter group and what they were built from."""
    __slots__ = ('key', 'params', 'tensors', 'chunks', 'n_tensors', 'n_chunks')


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0, weight_decay=0):
        if lr < 0.0:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if momentum < 0.0:
            raise ValueError('Invalid momentum value: %r' % (momentum,))
        if weight_decay < 0.0:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        # dampening and nesterov are torch.optim.SGD's keys at their off values: its step() reads them from a state dict of ours
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0, nesterov=False))
        names = {}
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group['params']):
                names[id(p)] = 'param_groups[%d][%d] %s' % (gi, pi, tuple(p.shape))
        self._names = names             # what a TypeError of step() calls a parameter (name_parameters: the model's own names)
        self._tables = {}               # group index -> _Table
        self._skipped = None            # device int32 [1], made with the first step
        self._guarded = 0               # guarded steps since the last settle()
        self._seen_skipped = 0          # the counter's value at the last settle()
        self._touched = {}              # id -> parameter updated by a guarded step since the last settle()
        self.uploads = 0                # how often a table went to the device
        self.launches = 0
        self.max_blocks = 0             # ymi_sgd_desc.max_blocks (0: the default cap)
        _LIVE.add(self)

    def name_parameters(self, named):
        """Use the model's own names in error messages: name_parameters(net.named_parameters())."""
        for n, p in named:
            if id(p) in self._names:
                self._names[id(p)] = n

    @staticmethod
    def _check(p, name):
        if p.dtype != torch.float32:
            raise TypeError('yolact_amd.optim.SGD: parameter %s is %s; the update kernel takes float32' % (name, p.dtype))
        if not p.is_cuda:
            raise TypeError('yolact_amd.optim.SGD: parameter %s lives on %s; the update kernel runs on the GPU and there is no CPU '
                            'path' % (name, p.device))
        if not p.is_contiguous():
            raise TypeError('yolact_amd.optim.SGD: parameter %s is not contiguous' % name)

    @property
    def skipped(self):
        """Device int32 [1]: how many guarded steps found a non-finite loss.  Reading it synchronises; step() never does."""
        if self._skipped is None:
            dev = next((p.device for g in self.param_groups for p in g['params']), None)
            self._skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        return self._skipped

    def zero_grad(self, set_to_none=False):
        """Keeps the gradient tensors by default: step() zeroes them in place, and a kept tensor keeps the uploaded table valid."""
        return super().zero_grad(set_to_none=set_to_none)

    def _table(self, gi, group, use_m):
        live = [p for p in group['params'] if p.grad is not None]
        for p in live:
            name = self._names.get(id(p), '?')
            self._check(p, name)
            g = p.grad
            if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.shape != p.shape:
                raise TypeError('yolact_amd.optim.SGD: the gradient of %s is not a contiguous float32 tensor of its shape on its device'
                                % name)
            if use_m and self.state[p].get('momentum_buffer') is None:      # absent, or torch's None of a state dict saved before a step
                self.state[p]['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if use_m:
                m = self.state[p]['momentum_buffer']
                if m.dtype != torch.float32 or m.device != p.device or not m.is_contiguous() or m.shape != p.shape:
                    raise TypeError('yolact_amd.optim.SGD: the momentum buffer of %s is not a contiguous float32 tensor of its shape on '
                                    'its device' % name)
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]['momentum_buffer'].data_ptr() if use_m else 0, p.numel())
                    for p in live)
        t = self._tables.get(gi)
        if t is not None and t.key == key:
            t.params = live             # the same storage, possibly through other tensor objects: the bump goes to the current ones
            return t
        t = _Table()
        t.key, t.params = key, live
        n = len(live)
        t.n_tensors = n
        recs = (L.SgdTensor * max(n, 1))()
        numel = (C.c_int64 * max(n, 1))()
        for i, (pp, gp, mp, cnt) in enumerate(key):
            recs[i] = L.SgdTensor(pp, gp, mp or None, cnt)
            numel[i] = cnt
        lib = L.lib()
        t.n_chunks = int(lib.ymi_sgd_plan(numel, n, None, 0))
        if t.n_chunks < 0:
            L.check(t.n_chunks, 'ymi_sgd_plan')
        chunks = (L.SgdChunk * max(t.n_chunks, 1))()
        lib.ymi_sgd_plan(numel, n, chunks, t.n_chunks)
        dev = live[0].device if live else self.skipped.device
        t.tensors = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(dev)
        t.chunks = torch.frombuffer(bytearray(bytes(chunks)), dtype=torch.uint8).to(dev)
        self._tables[gi] = t
        self.uploads += 1
        return t

    @torch.no_grad()
    def step(self, loss=None, zero_grad=True):
        """One launch per parameter group.  `loss`: a device scalar; when it is not finite nothing is updated and `skipped` grows by
        one (never read here).  zero_grad: the gradients are zeroed in the same pass, applied or skipped.  Parameters whose .grad is
        None are passed over, as torch does."""
        if loss is not None:
            if not torch.is_tensor(loss) or not loss.is_cuda or loss.dtype != torch.float32 or loss.numel() != 1:
                raise TypeError('yolact_amd.optim.SGD.step: loss must be a float32 scalar on the GPU')
            loss = loss.detach()
        lib = L.lib()
        counted = False                 # `skipped` counts STEPS: only the step's first launch is handed the counter
        for gi, group in enumerate(self.param_groups):
            mom = float(group['momentum'])
            if mom < 0:
                raise ValueError('Invalid momentum value: %r' % (mom,))
            if group.get('dampening', 0) or group.get('nesterov', False) or group.get('maximize', False):
                raise ValueError('yolact_amd.optim.SGD: dampening, nesterov and maximize are not offered')
            t = self._table(gi, group, mom > 0)
            if not t.params:
                continue
            dev = t.params[0].device
            d = L.SgdDesc()
            d.tensors, d.chunks = t.tensors.data_ptr(), t.chunks.data_ptr()
            d.n_tensors, d.n_chunks = t.n_tensors, t.n_chunks
            d.lr, d.momentum, d.weight_decay = float(group['lr']), mom, float(group['weight_decay'])     # c_float rounds once
            d.zero_grad = 1 if zero_grad else 0
            d.max_blocks = int(self.max_blocks)
            if loss is not None:
                if loss.device != dev:
                    raise TypeError('yolact_amd.optim.SGD.step: loss lives on %s, the parameters on %s' % (loss.device, dev))
                d.loss = loss.data_ptr()
                if not counted:
                    if self.skipped.device != dev:
                        raise TypeError('yolact_amd.optim.SGD.step: the skipped counter lives on %s, the parameters on %s'
                                        % (self.skipped.device, dev))
                    d.skipped = self.skipped.data_ptr()
                    counted = True
            with torch.cuda.device(dev):
                L.check(lib.ymi_sgd_step_f32(C.byref(d), L.stream_ptr()), 'ymi_sgd_step_f32')
            self.launches += 1
            if loss is None:
                torch.autograd.graph.increment_version(t.params)
            else:
                for p in t.params:
                    self._touched[id(p)] = p
                    _guarded_writes[p] = _guarded_writes.get(p, 0) + 1
        if counted:
            global _outstanding
            self._guarded += 1
            _outstanding += 1
        return None

    def settle(self):
        """Reads `skipped` (this synchronises) and, when a guarded step since the last call was applied, bumps the version counter of
        the parameters those steps covered.  -> how many of them were applied."""
        if not self._guarded:
            return 0
        global _outstanding
        now = int(self.skipped.item())
        applied = self._guarded - (now - self._seen_skipped)
        _outstanding = max(0, _outstanding - self._guarded)
        self._seen_skipped, self._guarded = now, 0
        touched, self._touched = list(self._touched.values()), {}
        if applied > 0 and touched:
            torch.autograd.graph.increment_version(touched)
        return applied
