"""ymi_sgd_step_f32 and yolact_amd.optim.SGD on the GPU: bit-equal to the numpy fp32 restatement of the contract on every path of the
kernel, the device-side guard, torch.optim.SGD and ours both inside one derived bound of an fp64 evaluation, and the optimiser's table
upload, version bumps and handling of parameters without gradients."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_ref as T  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.optim import SGD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def keep_the_global_cfg():
    saved = yolact_amd.config.cfg.copy()
    yield
    yolact_amd.config.cfg.replace(saved)
K = L.SGD_CHUNK
SIZES = [1, 3, 4, 5, K - 1, K, K + 1, 2 * K + 3]
GUARD = 8
SENTINEL = 12345.0
HYPER = [(0.9, 5e-4), (0.0, 5e-4), (0.9, 0.0), (0.0, 0.0)]
LR = 1e-3


class Slab:
    """n floats `shift` elements into a 16-byte aligned buffer, a sentinel band before and behind them."""

    def __init__(self, values, shift=0):
        n = values.numel()
        self.buf = torch.full((GUARD + shift + n + GUARD,), SENTINEL, device=DEV)
        self.t = self.buf[GUARD + shift: GUARD + shift + n]
        self.t.copy_(values)
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (4 * shift) % 16

    def host(self):
        b = self.buf.cpu().numpy()
        n = self.t.numel()
        lo = len(b) - n - GUARD
        assert (b[:lo] == SENTINEL).all() and (b[lo + n:] == SENTINEL).all(), 'written outside the tensor'
        return b[lo: lo + n].copy()


def make_tensors(gen, with_m):
    """The tensor list of the exactness test: SIZES, then the scalar path: p, g or m one element off 16-byte alignment."""
    spec = [(n, (0, 0, 0)) for n in SIZES] + [(K + 5, (1, 0, 0)), (7, (0, 1, 0))] + ([(9, (0, 0, 1))] if with_m else [])
    out = []
    for n, (sp, sg, sm) in spec:
        p = Slab(torch.randn(n, generator=gen), sp)
        g = Slab(torch.zeros(n), sg)
        m = Slab(torch.zeros(n), sm) if with_m else None
        out.append((p, g, m))
    return out


def upload(tensors):
    n = len(tensors)
    recs = (L.SgdTensor * n)()
    numel = (C.c_int64 * n)()
    for i, (p, g, m) in enumerate(tensors):
        recs[i] = L.SgdTensor(p.t.data_ptr(), g.t.data_ptr(), m.t.data_ptr() if m is not None else None, p.t.numel())
        numel[i] = p.t.numel()
    lib = L.lib()
    nc = int(lib.ymi_sgd_plan(numel, n, None, 0))
    chunks = (L.SgdChunk * nc)()
    assert lib.ymi_sgd_plan(numel, n, chunks, nc) == nc
    dt = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV)
    dc = torch.frombuffer(bytearray(bytes(chunks)), dtype=torch.uint8).to(DEV)
    return recs, dt, dc, n, nc


def launch(table, lr, mom, wd, zero_grad=1, loss=None, skipped=None, max_blocks=0):
    recs, dt, dc, n, nc = table
    d = L.SgdDesc()
    d.tensors, d.chunks, d.tensors_host = dt.data_ptr(), dc.data_ptr(), recs
    d.n_tensors, d.n_chunks = n, nc
    d.lr, d.momentum, d.weight_decay = lr, mom, wd
    d.zero_grad, d.max_blocks = zero_grad, max_blocks
    d.loss = loss.data_ptr() if loss is not None else None
    d.skipped = skipped.data_ptr() if skipped is not None else None
    L.check(L.lib().ymi_sgd_step_f32(C.byref(d), L.stream_ptr()), 'ymi_sgd_step_f32')
    torch.cuda.synchronize()


@pytest.mark.parametrize('max_blocks', [0, 1])
@pytest.mark.parametrize('mom,wd', HYPER)
def test_three_steps_bit_equal_to_numpy(mom, wd, max_blocks):
    gen = torch.Generator().manual_seed(17)
    tensors = make_tensors(gen, mom > 0)
    table = upload(tensors)
    want = [(p.host(), np.zeros(p.t.numel(), np.float32)) for p, _, _ in tensors]
    for step in range(3):
        grads = [torch.randn(p.t.numel(), generator=gen) * (0.1 + step) for p, _, _ in tensors]
        for (p, g, m), gr in zip(tensors, grads):
            g.t.copy_(gr)
        launch(table, LR, mom, wd, max_blocks=max_blocks)
        for i, ((p, g, m), gr) in enumerate(zip(tensors, grads)):
            wp, wm = T.sgd_step_np(want[i][0], gr.numpy(), want[i][1], LR, mom, wd)
            want[i] = (wp, wm)
            gp = p.host()
            assert gp.tobytes() == wp.tobytes(), (step, i, p.t.numel(), int((gp != wp).sum()))
            if m is not None:
                assert m.host().tobytes() == wm.tobytes(), (step, i, p.t.numel())
            gg = g.host()
            assert gg.tobytes() == np.zeros_like(gg).tobytes(), (step, i)        # +0.0, every element
    assert any((w[0] != 0).all() for w in want)


def test_gradients_kept_without_zero_grad():
    gen = torch.Generator().manual_seed(18)
    tensors = make_tensors(gen, True)
    table = upload(tensors)
    grads = [torch.randn(p.t.numel(), generator=gen) for p, _, _ in tensors]
    for (p, g, m), gr in zip(tensors, grads):
        g.t.copy_(gr)
    before = [p.host() for p, _, _ in tensors]
    launch(table, LR, 0.9, 5e-4, zero_grad=0)
    for (p, g, m), gr, b in zip(tensors, grads, before):
        assert g.host().tobytes() == gr.numpy().tobytes()
        wp, wm = T.sgd_step_np(b, gr.numpy(), np.zeros_like(b), LR, 0.9, 5e-4)
        assert p.host().tobytes() == wp.tobytes() and m.host().tobytes() == wm.tobytes()


@pytest.mark.parametrize('bad', [float('inf'), float('-inf'), float('nan')])
def test_guard_skips_and_counts(bad):
    gen = torch.Generator().manual_seed(19)
    tensors = make_tensors(gen, True)
    table = upload(tensors)
    skipped = torch.full((1,), 5, dtype=torch.int32, device=DEV)

    def set_grads():
        grads = [torch.randn(p.t.numel(), generator=gen) for p, _, _ in tensors]
        for (p, g, m), gr in zip(tensors, grads):
            g.t.copy_(gr)
        return grads
    grads = set_grads()
    start = [p.host() for p, _, _ in tensors]
    launch(table, LR, 0.9, 5e-4, loss=torch.tensor(1.5, device=DEV), skipped=skipped)      # a finite loss: applied, not counted
    assert int(skipped.item()) == 5
    state = []
    for (p, g, m), gr, p0 in zip(tensors, grads, start):
        wp, wm = T.sgd_step_np(p0, gr.numpy(), np.zeros_like(p0), LR, 0.9, 5e-4)
        state.append((p.host(), m.host()))
        assert state[-1][0].tobytes() == wp.tobytes() and state[-1][1].tobytes() == wm.tobytes() and not g.host().any()
    set_grads()
    launch(table, LR, 0.9, 5e-4, loss=torch.tensor(bad, device=DEV), skipped=skipped)
    assert int(skipped.item()) == 6
    for (p, g, m), (bp, bm) in zip(tensors, state):
        assert p.host().tobytes() == bp.tobytes() and m.host().tobytes() == bm.tobytes()
        gg = g.host()
        assert gg.tobytes() == np.zeros_like(gg).tobytes()
    kept = set_grads()
    launch(table, LR, 0.9, 5e-4, zero_grad=0, loss=torch.tensor(bad, device=DEV), skipped=skipped)      # skipped, nothing to zero
    assert int(skipped.item()) == 7
    for (p, g, m), (bp, bm), gr in zip(tensors, state, kept):
        assert p.host().tobytes() == bp.tobytes() and m.host().tobytes() == bm.tobytes() and g.host().tobytes() == gr.numpy().tobytes()
    launch(table, LR, 0.9, 5e-4, loss=torch.tensor(bad, device=DEV), skipped=None)                       # no counter: still skipped
    for (p, g, m), (bp, bm) in zip(tensors, state):
        assert p.host().tobytes() == bp.tobytes() and m.host().tobytes() == bm.tobytes() and not g.host().any()


def step64(p, g, m, lr, mom, wd):
    """The step in fp64 from fp32 inputs and fp32-rounded hyper-parameters -> (p', m', b_p, b_m): the bounds that test_ours_and_torch_within_the_fp64_bound
    derives."""
    lr, mom, wd = (float(np.float32(v)) for v in (lr, mom, wd))
    p, g, m = p.astype(np.float64), g.astype(np.float64), m.astype(np.float64)
    d = g + wd * p
    m1 = mom * m + d
    p1 = p - lr * m1
    u = 2.0 ** -23
    b_m = u * (np.abs(d) + np.abs(m1) + np.abs(mom * m) + np.abs(wd * p))
    b_p = u * ((np.abs(p1) + np.abs(p)) / 2 + np.abs(lr * m1)) + 1.01 * lr * b_m
    return p1, m1, b_p, b_m


def ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_ours_and_torch_within_the_fp64_bound():
    """After each of 3 steps, ours and torch.optim.SGD (GPU) lie within b_p / b_m of the fp64 evaluation of that step from the fp32 state
    each of them started it from:
        b_m = 2^-23 (|d| + |m'| + |mom m| + |wd p|)                  one rounding each of wd p, d, mom m and m'
        b_p = 2^-23 ((|p'| + |p|) / 2 + |lr m'|) + 1.01 lr b_m       the roundings of lr m' and p', and m's error carried through lr
    (2^-23 is twice the unit roundoff: an FMA-contracted evaluation, torch's, rounds less often and fits too).  The largest
    ours - torch difference is printed in ulps."""
    gen = torch.Generator().manual_seed(23)
    n = 2 * K + 3
    lr, mom, wd = 1e-3, 0.9, 5e-4
    scale = 10.0 ** (torch.rand(n, generator=gen) * 7 - 4)                      # seven decades
    p0 = torch.randn(n, generator=gen) * scale
    ours_p = torch.nn.Parameter(p0.clone().to(DEV))
    their_p = torch.nn.Parameter(p0.clone().to(DEV))
    ours = SGD([ours_p], lr=lr, momentum=mom, weight_decay=wd)
    theirs = torch.optim.SGD([their_p], lr=lr, momentum=mom, weight_decay=wd)
    worst = {'ours p': 0.0, 'ours m': 0.0, 'torch p': 0.0, 'torch m': 0.0}
    diff_ulps = 0
    for step in range(3):
        g = torch.randn(n, generator=gen) * scale * (1 + step)
        for name, opt, p in (('ours', ours, ours_p), ('torch', theirs, their_p)):
            m_before = opt.state[p]['momentum_buffer'].cpu().numpy() if 'momentum_buffer' in opt.state[p] else np.zeros(n, np.float32)
            p_before = p.detach().cpu().numpy()
            p.grad = g.clone().to(DEV)
            opt.step()
            torch.cuda.synchronize()
            p1, m1, b_p, b_m = step64(p_before, g.numpy(), m_before, lr, mom, wd)
            got_p, got_m = p.detach().cpu().numpy(), opt.state[p]['momentum_buffer'].cpu().numpy()
            rp = float((np.abs(got_p - p1) / b_p).max())
            rm = float((np.abs(got_m - m1) / np.maximum(b_m, 1e-300)).max())
            print('step %d %s: p error / bound %.3f, m error / bound %.3f' % (step, name, rp, rm))
            worst[name + ' p'], worst[name + ' m'] = max(worst[name + ' p'], rp), max(worst[name + ' m'], rm)
        theirs.zero_grad()
        diff_ulps = max(diff_ulps, int(ulps(ours_p.detach().cpu().numpy(), their_p.detach().cpu().numpy()).max()))
        print('step %d: largest ours - torch difference in p %d ulps' % (step, diff_ulps))
    print('worst ratios', worst, 'largest ours - torch difference', diff_ulps, 'ulps')
    for k, v in worst.items():
        assert v <= 1.0, (k, v)


def small_params(gen, sizes=(5, K + 1, 12)):
    return [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in sizes]


def test_table_uploaded_once_and_again_when_a_grad_goes():
    gen = torch.Generator().manual_seed(29)
    ps = small_params(gen)
    opt = SGD(ps, lr=LR, momentum=0.9, weight_decay=5e-4)
    want = [(p.detach().cpu().numpy(), np.zeros(p.numel(), np.float32)) for p in ps]
    for step in range(3):
        grads = [torch.randn(p.numel(), generator=gen) for p in ps]
        for p, g in zip(ps, grads):
            if p.grad is None:
                p.grad = g.to(DEV)
            else:
                p.grad.copy_(g)                      # what backward() does to a kept, zeroed gradient: accumulate in place
        opt.step(torch.tensor(0.5, device=DEV))
        want = [T.sgd_step_np(w[0], g.numpy(), w[1], LR, 0.9, 5e-4) for w, g in zip(want, grads)]
    torch.cuda.synchronize()
    assert opt.uploads == 1 and opt.launches == 3
    for p, w in zip(ps, want):
        assert p.detach().cpu().numpy().tobytes() == w[0].tobytes()
        assert opt.state[p]['momentum_buffer'].cpu().numpy().tobytes() == w[1].tobytes()
        assert not p.grad.cpu().numpy().any()
    assert int(opt.skipped.item()) == 0
    # one parameter loses its gradient: it is passed over bit for bit, and the table is built again
    ps[1].grad = None
    frozen = ps[1].detach().cpu().numpy().copy()
    frozen_m = opt.state[ps[1]]['momentum_buffer'].cpu().numpy().copy()
    grads = [torch.randn(p.numel(), generator=gen) for p in ps]
    for p, g in zip(ps, grads):
        if p.grad is not None:
            p.grad.copy_(g)
    opt.step()
    torch.cuda.synchronize()
    assert opt.uploads == 2 and opt.launches == 4
    assert ps[1].detach().cpu().numpy().tobytes() == frozen.tobytes()
    assert opt.state[ps[1]]['momentum_buffer'].cpu().numpy().tobytes() == frozen_m.tobytes()
    for i in (0, 2):
        w = T.sgd_step_np(want[i][0], grads[i].numpy(), want[i][1], LR, 0.9, 5e-4)
        assert ps[i].detach().cpu().numpy().tobytes() == w[0].tobytes()
    opt.zero_grad()                                   # keeps the tensors
    assert ps[0].grad is not None and not ps[0].grad.any()


def test_refusals_on_the_gpu():
    p = torch.nn.Parameter(torch.zeros(4, 6, device=DEV).t())           # not contiguous
    p.grad = torch.ones(6, 4, device=DEV)
    with pytest.raises(TypeError, match='not contiguous'):
        SGD([p], lr=LR).step()
    q = torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))
    q.grad = torch.ones(4, device=DEV, dtype=torch.float16)
    with pytest.raises(TypeError, match='float16'):
        SGD([q], lr=LR).step()
    r = torch.nn.Parameter(torch.zeros(4, device=DEV))
    r.grad = torch.ones(4, device=DEV)
    with pytest.raises(TypeError, match='loss'):
        SGD([r], lr=LR).step(loss=torch.tensor(1.0))                     # a host loss would need a host read
    assert not r.detach().cpu().any()


def test_param_stamp_follows_applied_steps():
    yolact_amd.set_cfg('yolact_resnet50_config')
    from yolact_amd.yolact import Yolact
    torch.manual_seed(1)
    net = Yolact().to(DEV)
    ps = list(net.prediction_layers.parameters())
    opt = SGD(ps, lr=LR, momentum=0.9, weight_decay=5e-4)

    def grads():
        for p in ps:
            if p.grad is None:
                p.grad = torch.ones_like(p)
            else:
                p.grad.fill_(1.0)
    before = [p.detach().clone() for p in ps]
    s0 = net._param_stamp()
    grads()
    opt.step(torch.tensor(float('inf'), device=DEV))
    assert net._param_stamp() == s0                                      # skipped: nothing changed, no plan needs rebuilding
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, ps))
    assert int(opt.skipped.item()) == 1
    grads()
    opt.step(torch.tensor(2.0, device=DEV))
    s1 = net._param_stamp()
    assert s1 != s0 and net._param_stamp() == s1                         # applied: bumped once it is settled, and only once
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, ps))
    grads()
    opt.step(torch.tensor(float('nan'), device=DEV))
    grads()
    opt.step(torch.tensor(1.0, device=DEV))
    assert net._param_stamp() != s1                                      # one applied step among the outstanding ones is enough
    s2 = net._param_stamp()
    grads()
    opt.step()                                                           # no guard: bumped at once
    assert sum(p._version for p in ps) != 0 and net._param_stamp() != s2
    assert int(opt.skipped.item()) == 2


def test_two_groups_count_steps_and_settle_right():
    """Two parameter groups, as in 'no weight decay on biases': `skipped` counts steps, not launches, and one applied step among the
    outstanding guarded ones is seen by the stamp although another one was skipped."""
    yolact_amd.set_cfg('yolact_resnet50_config')
    from yolact_amd.yolact import Yolact
    torch.manual_seed(2)
    net = Yolact().to(DEV)
    named = list(net.prediction_layers.named_parameters())
    decay = [p for n, p in named if not n.endswith('bias')]
    plain = [p for n, p in named if n.endswith('bias')]
    assert decay and plain
    opt = SGD([{'params': decay, 'weight_decay': 5e-4}, {'params': plain, 'weight_decay': 0.0}], lr=LR, momentum=0.9)
    ps = decay + plain

    def grads():
        for p in ps:
            if p.grad is None:
                p.grad = torch.ones_like(p)
            else:
                p.grad.fill_(1.0)
    before = [p.detach().clone() for p in ps]
    s0 = net._param_stamp()
    grads()
    opt.step(torch.tensor(1.0, device=DEV))                              # applied
    grads()
    opt.step(torch.tensor(float('inf'), device=DEV))                     # skipped
    assert opt.launches == 4
    assert net._param_stamp() != s0                                      # the weights changed: the plans must notice
    assert int(opt.skipped.item()) == 1                                  # one step, two launches
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, ps))
    s1 = net._param_stamp()
    for _ in range(2):
        grads()
        opt.step(torch.tensor(float('nan'), device=DEV))
    assert net._param_stamp() == s1 and int(opt.skipped.item()) == 3     # two skipped steps: nothing to notice


def test_momentum_buffer_none_counts_as_absent():
    gen = torch.Generator().manual_seed(31)
    p = torch.nn.Parameter(torch.randn(9, generator=gen).to(DEV))
    g = torch.randn(9, generator=gen)
    p.grad = g.to(DEV)
    opt = SGD([p], lr=LR, momentum=0.9, weight_decay=5e-4)
    opt.state[p]['momentum_buffer'] = None                               # what torch.optim.SGD saves before its first step
    p0 = p.detach().cpu().numpy()
    opt.step()
    wp, wm = T.sgd_step_np(p0, g.numpy(), np.zeros(9, np.float32), LR, 0.9, 5e-4)
    assert p.detach().cpu().numpy().tobytes() == wp.tobytes()
    assert opt.state[p]['momentum_buffer'].cpu().numpy().tobytes() == wm.tobytes()


def test_dcn_forward_uses_the_stepped_weights():
    """dcn_v2 keeps packed filters keyed on the parameters' version counters, and a guarded step's bump waits for settle(): the next
    forward must still run on the new weights (optim.guarded_writes is in the key), with no Yolact around to settle anything."""
    from yolact_amd.dcn_v2 import DCN
    torch.manual_seed(7)
    dcn = DCN(32, 32, 3, stride=1, padding=1).to(DEV)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, 32, 9, 7, generator=gen).to(DEV)
    up = torch.randn(2, 32, 9, 7, generator=gen).to(DEV)
    opt = SGD(dcn.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)

    def fresh():
        other = DCN(32, 32, 3, stride=1, padding=1).to(DEV)
        other.load_state_dict(dcn.state_dict())
        with torch.no_grad():
            return other(x)
    y0 = dcn(x)
    assert torch.equal(y0.detach(), fresh())
    (y0 * up).sum().backward()
    versions = [p._version for p in dcn.parameters()]
    opt.step(torch.tensor(float('inf'), device=DEV))                     # skipped: the same output
    y_skipped = dcn(x)
    assert torch.equal(y_skipped.detach(), y0.detach())
    (y_skipped * up).sum().backward()
    opt.step(torch.tensor(3.0, device=DEV))                              # applied, not settled
    assert [p._version for p in dcn.parameters()] == versions
    y1 = dcn(x)
    assert not torch.equal(y1.detach(), y0.detach())
    assert torch.equal(y1.detach(), fresh())
    (y1 * up).sum().backward()                                           # nothing bumped under the saved tensors: backward runs
    with torch.no_grad():
        assert torch.equal(dcn(x), y1.detach())
    assert int(opt.skipped.item()) == 1
