"""The training step's host side: the C ABI of the SGD update (header, binding, chunk plan, argument errors), the learning-rate schedule,
autoscale, the optimiser's refusals and state dicts, and Yolact.init_weights against the reference's own.  No GPU."""
import ctypes as C
import json
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_train_ref as H  # noqa: E402
import train_step_ref as T  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.optim import SGD  # noqa: E402
from yolact_amd.training import autoscale, lr_at  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARG = -1


@pytest.fixture(autouse=True)
def keep_the_global_cfg():
    """Tests here select and edit yolact_amd.config.cfg: whatever they leave, the next test finds what this one found."""
    saved = yolact_amd.config.cfg.copy()
    yield
    yolact_amd.config.cfg.replace(saved)


def test_header_and_binding():
    hdr = open(os.path.join(ROOT, 'include', 'yolact_amd.h')).read()
    assert re.search(r'^int ymi_sgd_step_f32\(const ymi_sgd_desc \*d, void \*stream\);', hdr, re.M)
    assert re.search(r'^int64_t ymi_sgd_plan\(const int64_t \*numel, int n, ymi_sgd_chunk \*out, int64_t cap\);', hdr, re.M)
    chunk = int(re.search(r'^#define YMI_SGD_CHUNK (\d+)', hdr, re.M).group(1))
    assert chunk == L.SGD_CHUNK and chunk % 4 == 0 and chunk > 0
    assert int(re.search(r'^#define YMI_ABI_VERSION (\d+)', hdr, re.M).group(1)) == 9 == L.ABI_VERSION
    names = {s for s, _, _ in L.SYMBOLS}
    assert {'ymi_sgd_step_f32', 'ymi_sgd_plan'} <= names
    lib = L.lib()
    assert lib.ymi_abi_version() == 9
    assert lib.ymi_sgd_step_f32.argtypes[0]._type_ is L.SgdDesc
    # the C layouts: {3 pointers, int64}, {int32, pad, int64}, {5 pointers, 2 int32, 3 float, 3 int32}
    assert C.sizeof(L.SgdTensor) == 32 and C.sizeof(L.SgdChunk) == 16 and L.SgdChunk.first.offset == 8
    assert C.sizeof(L.SgdDesc) == 5 * 8 + 8 * 4 and L.SgdDesc.n_tensors.offset == 40


def plan(numel, cap=None, write=True):
    lib = L.lib()
    arr = (C.c_int64 * max(len(numel), 1))(*numel)
    n = int(lib.ymi_sgd_plan(arr, len(numel), None, 0))
    if not write:
        return n
    cap = n if cap is None else cap
    out = (L.SgdChunk * max(cap, 1))()
    for c in out:
        c.tensor, c.first = -7, -7
    assert int(lib.ymi_sgd_plan(arr, len(numel), out, cap)) == n
    return [(c.tensor, c.first) for c in out[:cap]]


def test_plan_exact_tables():
    K = L.SGD_CHUNK
    numel = [0, 1, K - 1, K, K + 1, 2 * K + 3]
    want = [(1, 0), (2, 0), (3, 0), (4, 0), (4, K), (5, 0), (5, K), (5, 2 * K)]
    assert plan(numel, write=False) == len(want)
    assert plan(numel) == want
    assert plan(numel, cap=3) == want[:3]                       # never past `cap`
    assert plan([]) == [] and plan([0, 0]) == []
    assert plan([3 * K]) == [(0, 0), (0, K), (0, 2 * K)]
    lib = L.lib()
    one = (C.c_int64 * 1)(5)
    bad = (C.c_int64 * 2)(5, -1)
    out = (L.SgdChunk * 4)()
    assert lib.ymi_sgd_plan(None, 1, None, 0) == EARG
    assert lib.ymi_sgd_plan(one, -1, None, 0) == EARG
    assert lib.ymi_sgd_plan(bad, 2, None, 0) == EARG
    assert lib.ymi_sgd_plan(one, 1, out, -1) == EARG


def good_desc(host):
    d = L.SgdDesc()
    d.tensors, d.chunks = 0x1000, 0x2000        # never dereferenced: every case below is refused before the launch
    d.tensors_host = host
    d.n_tensors, d.n_chunks = 1, 1
    d.lr, d.momentum, d.weight_decay = 1e-3, 0.9, 5e-4
    return d


EARG_CASES = {
    'tensors NULL': lambda d, h: setattr(d, 'tensors', None),
    'chunks NULL': lambda d, h: setattr(d, 'chunks', None),
    'n_tensors < 0': lambda d, h: setattr(d, 'n_tensors', -1),
    'n_chunks < 0': lambda d, h: setattr(d, 'n_chunks', -1),
    'max_blocks < 0': lambda d, h: setattr(d, 'max_blocks', -1),
    'momentum < 0': lambda d, h: setattr(d, 'momentum', -0.5),
    'momentum nan': lambda d, h: setattr(d, 'momentum', float('nan')),
    'm NULL with momentum > 0': lambda d, h: setattr(h[0], 'm', None),
    'p NULL': lambda d, h: setattr(h[0], 'p', None),
    'g NULL': lambda d, h: setattr(h[0], 'g', None),
    'n < 0': lambda d, h: setattr(h[0], 'n', -1),
}


@pytest.mark.parametrize('case', sorted(EARG_CASES))
def test_step_argument_errors(case):
    host = (L.SgdTensor * 1)(L.SgdTensor(0x3000, 0x4000, 0x5000, 8))
    d = good_desc(host)
    EARG_CASES[case](d, host)
    assert L.lib().ymi_sgd_step_f32(C.byref(d), None) == EARG, case


def test_step_null_descriptor():
    assert L.lib().ymi_sgd_step_f32(None, None) == -3


def lr_literal(it):
    """train.py:295-301 for yolact_base_config, written out."""
    if it <= 500:
        return (1e-3 - 1e-4) * (it / 500) + 1e-4
    steps = (280000, 600000, 700000, 750000)
    return 1e-3 * (0.1 ** len([s for s in steps if it >= s]))


def test_lr_at_yolact_base():
    cfg = yolact_amd.CONFIGS['yolact_base_config']
    assert (cfg.lr, cfg.momentum, cfg.decay, cfg.gamma) == (1e-3, 0.9, 5e-4, 0.1)
    assert (cfg.lr_warmup_init, cfg.lr_warmup_until, cfg.max_iter, cfg.freeze_bn) == (1e-4, 500, 800000, False)
    assert tuple(cfg.lr_steps) == (280000, 600000, 700000, 750000)
    for it in (0, 1, 250, 500, 501, 279999, 280000, 600000, 750000):
        assert lr_at(it, cfg) == lr_literal(it), it
    assert lr_at(0, cfg) == 1e-4 and lr_at(501, cfg) == 1e-3 and lr_at(279999, cfg) == 1e-3
    assert lr_at(280000, cfg) == 1e-3 * 0.1 and lr_at(750000, cfg) == 1e-3 * 0.1 ** 4
    assert lr_at(501, cfg, lr=2e-3, gamma=0.5) == 2e-3 and lr_at(280000, cfg, lr=2e-3, gamma=0.5) == 1e-3
    for name, c in yolact_amd.CONFIGS.items():      # every shipped config is made from yolact_base_config (data/config.py:667-668)
        assert tuple(c.lr_steps) == (280000, 600000, 700000, 750000) and c.max_iter == 800000, name


@pytest.mark.parametrize('batch', [4, 8, 16])
def test_autoscale(batch):
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    assert autoscale(cfg, batch) is cfg
    f = batch / 8
    if batch == 8:
        assert cfg.lr == 1e-3 and cfg.max_iter == 800000 and tuple(cfg.lr_steps) == (280000, 600000, 700000, 750000)
    else:
        assert cfg.lr == 1e-3 * f and cfg.max_iter == 800000 // f and list(cfg.lr_steps) == [x // f for x in (280000, 600000, 700000, 750000)]
    assert {4: (5e-4, 1600000, 560000), 8: (1e-3, 800000, 280000), 16: (2e-3, 400000, 140000)}[batch] == \
        (cfg.lr, cfg.max_iter, cfg.lr_steps[0])
    assert yolact_amd.CONFIGS['yolact_base_config'].lr == 1e-3      # the shipped config is untouched


def test_sgd_refuses_a_cpu_parameter():
    p = torch.nn.Parameter(torch.zeros(4, 3))
    p.grad = torch.ones(4, 3)
    opt = SGD([p], lr=0.1, momentum=0.9)
    opt.name_parameters([('head.weight', p)])
    with pytest.raises(TypeError, match='head.weight'):
        opt.step()
    assert bool((p == 0).all())
    with pytest.raises(TypeError, match=r'param_groups\[0\]\[0\]'):
        q = torch.nn.Parameter(torch.zeros(2))
        q.grad = torch.ones(2)
        SGD([q], lr=0.1).step()
    for bad in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.1), dict(lr=0.1, weight_decay=-1.0)):
        with pytest.raises(ValueError):
            SGD([p], **bad)


def test_state_dict_round_trip_with_torch_sgd():
    gen = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(7, 3, generator=gen)), torch.nn.Parameter(torch.randn(5, generator=gen))]
    theirs = torch.optim.SGD(ps, lr=1e-2, momentum=0.9, weight_decay=5e-4)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen)
    theirs.step()
    sd = theirs.state_dict()
    ours = SGD(ps, lr=1.0)
    ours.load_state_dict(sd)
    g = ours.param_groups[0]
    assert (g['lr'], g['momentum'], g['weight_decay']) == (1e-2, 0.9, 5e-4)
    for p in ps:
        assert torch.equal(ours.state[p]['momentum_buffer'], theirs.state[p]['momentum_buffer'])
    for group in ours.param_groups:      # the reference's set_lr (train.py:388-391)
        group['lr'] = 3e-3
    back = torch.optim.SGD(ps, lr=1.0)
    back.load_state_dict(ours.state_dict())
    assert back.param_groups[0]['lr'] == 3e-3 and back.param_groups[0]['momentum'] == 0.9
    for p in ps:
        assert torch.equal(back.state[p]['momentum_buffer'], theirs.state[p]['momentum_buffer'])
    back.step()                           # and torch goes on from it
    fresh = torch.optim.SGD(ps, lr=1.0)    # a state dict of ours that never saw torch's: torch steps from it too
    fresh.load_state_dict(SGD(ps, lr=2e-3, momentum=0.9, weight_decay=5e-4).state_dict())
    assert (fresh.param_groups[0]['lr'], fresh.param_groups[0]['dampening'], fresh.param_groups[0]['nesterov']) == (2e-3, 0, False)
    fresh.step()
    bad = SGD(ps, lr=1e-3)
    bad.param_groups[0]['nesterov'] = True
    with pytest.raises(ValueError, match='nesterov'):
        bad.step()
    assert sorted(ours.state_dict()['state']) == sorted(sd['state'])
    assert set(ours.state_dict()['state'][0]) == {'momentum_buffer'}


def test_init_weights_matches_the_reference(tmp_path):
    """Yolact.init_weights on the backbone file and seed of tools/make_golden_init_weights.py: every tensor the golden covers has the bytes
    the reference's own init_weights left (tests/golden/init_weights.json holds their SHA-256)."""
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'init_weights.json')))
    yolact_amd.set_cfg('yolact_resnet50_config')
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    from yolact_amd.yolact import Yolact
    net = Yolact()
    path = str(tmp_path / 'backbone.pth')
    torch.save(T.backbone_file_state(net.backbone), path)
    net._plans['stale'] = object()
    torch.manual_seed(golden['seed'])
    net.init_weights(path)
    assert not net._plans                                           # the plans are dropped
    sd = net.state_dict()
    keys = T.init_digest_keys(net)
    assert sorted(keys) == sorted(golden['sha256'])
    assert any(k.startswith('backbone.layers.1.3.') for k in keys) and 'backbone.layers.1.2.conv1.weight' not in keys
    wrong = [k for k in keys if T.sha256(sd[k]) != golden['sha256'][k]]
    assert not wrong, wrong
    for k in keys:                                                  # zero biases outside the backbone
        if not k.startswith('backbone.') and k.endswith('.bias'):
            assert not sd[k].any(), k
    with pytest.raises(NotImplementedError):                        # still an eval-mode object
        net.train()


def test_freeze_bn_sets_requires_grad_only():
    yolact_amd.set_cfg('yolact_resnet50_config')
    from yolact_amd.yolact import Yolact
    net = Yolact()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 53
    net.freeze_bn()
    assert not any(m.weight.requires_grad or m.bias.requires_grad for m in bns) and not any(m.training for m in bns)
    assert net.backbone.conv1.weight.requires_grad
    net.freeze_bn(True)
    assert all(m.weight.requires_grad and m.bias.requires_grad for m in bns) and not any(m.training for m in bns)
