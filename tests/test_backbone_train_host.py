"""The train-mode ResNet stages on the CPU: the oracle of tests/backbone_train_ref.py is pinned to what the reference's own Bottleneck
class computed in both BatchNorm modes (tests/golden/backbone_train.npz, tools/make_golden_backbone_train.py), and the surface that
needs no GPU is checked: the ABI number, the BatchNorm workspace, argument validation of ymi_conv_dgrad_s2_nhwc_f32,
ymi_bn_fwd_nhwc_f32 and ymi_bn_bwd_nhwc_f32, the Python refusals.

Golden bar: every stored output, gradient and running statistic: rel_err <= 1e-6 for the fp32 and for the fp64 oracle, the bar of
tests/test_fpn_train_host.py.
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backbone_train_ref as R  # noqa: E402
from helpers import rel_err  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import modules as M  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

META, X, PARAMS, BLOCKS, UP, WANT = R.load_golden()
GOLDEN_BAR = 1e-6
ENULL, EARG, ESHAPE = -3, -1, -2
MODES = (('eval', False), ('train', True))
HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_golden_case_is_the_one_the_issue_describes():
    assert tuple(X.shape) == (2, 64, 9, 7) and tuple(UP.shape) == (2, 128, 5, 4)
    assert BLOCKS == [('0.', 2), ('1.', 1)]
    assert list(PARAMS) == ['0.' + n for n in R.block_param_names(True)] + ['1.' + n for n in R.block_param_names(False)]
    assert tuple(PARAMS['0.downsample.0.weight'].shape) == (128, 64, 1, 1) and tuple(PARAMS['1.conv1.weight'].shape) == (32, 128, 1, 1)
    leaves = [n for n in PARAMS if R.is_leaf_name(n)]
    stats = [n for n in PARAMS if not R.is_leaf_name(n)]
    assert len(leaves) == 7 + 14 and len(stats) == 14
    assert sorted(WANT['eval']) == sorted(['y', 'd_x'] + ['d_' + n for n in leaves])
    assert sorted(WANT['train']) == sorted(['y', 'd_x'] + ['d_' + n for n in leaves] + ['new_' + n for n in stats])
    for mode, _ in MODES:
        assert tuple(WANT[mode]['y'].shape) == (2, 128, 5, 4) and tuple(WANT[mode]['d_x'].shape) == (2, 64, 9, 7)
        for k, v in WANT[mode].items():
            assert v.dtype == torch.float32 and bool(v.ne(0).any()), (mode, k)
    for t in [X, UP] + list(PARAMS.values()):
        assert torch.equal(t.half().float(), t)                                          # the fp16-exact grids
    for n in stats:                                                                      # non-trivial running statistics, which move
        assert not torch.equal(PARAMS[n], torch.zeros_like(PARAMS[n])) and not torch.equal(PARAMS[n], torch.ones_like(PARAMS[n]))
        assert not torch.equal(WANT['train']['new_' + n], PARAMS[n])
    assert META['searched'] == 64 and 1 <= META['qualified'] <= 64 and 1 <= META['seed'] <= 64
    assert os.path.getsize(os.path.join(HERE, 'golden', 'backbone_train.npz')) <= 652222


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('mode', MODES, ids=['eval', 'train'])
def test_oracle_equals_the_reference(mode, dtype):
    name, train = mode
    r = R.run_ref(X, PARAMS, BLOCKS, UP, train, dtype)
    assert sorted(k for k in r if not k.startswith('_') and (train or not k.startswith('new_'))) == sorted(WANT[name])
    for k in WANT[name]:
        e = rel_err(r[k], WANT[name][k])
        print('%s %s %s: %.3e' % (name, dtype, k, e))
        assert e <= GOLDEN_BAR, (k, e)


def test_golden_tells_a_wrong_oracle_apart():
    """The stride on conv1 instead of conv2 (the other ResNet flavour), or the biased variance in the running update: not met."""
    for name, train in MODES:
        r = R.run_ref(X, PARAMS, BLOCKS, UP, train, torch.float64, stride_on_conv1=True)
        assert r['y'].shape == WANT[name]['y'].shape and rel_err(r['y'], WANT[name]['y']) > 1e-3
    r = R.run_ref(X, PARAMS, BLOCKS, UP, True, torch.float64, unbiased_running=False)
    assert rel_err(r['y'], WANT['train']['y']) <= GOLDEN_BAR
    assert rel_err(r['new_0.bn1.running_mean'], WANT['train']['new_0.bn1.running_mean']) <= GOLDEN_BAR
    for n in PARAMS:
        if n.endswith('running_var'):
            assert rel_err(r['new_' + n], WANT['train']['new_' + n]) > 1e-4, n


def test_margins_of_the_golden_case():
    for name, train in MODES:
        m = R.relu_margins(X, PARAMS, BLOCKS, UP, train)
        print('golden %s, tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % ((name,) + R.tightest(m)))
        assert len(m) == 6
        R.assert_margins(m)
        r64, r32 = (R.run_ref(X, PARAMS, BLOCKS, UP, train, dt) for dt in (torch.float64, torch.float32))
        assert max(rel_err(r32[k], r64[k]) for k in WANT[name]) <= 1e-6


def test_an_upstream_gradient_per_block_output():
    """run_ref's ups: with zeros everywhere but at the last output it is the single-up result; a gradient at the first block's output
    as well adds exactly the gradient of that term (the total is linear in the ups), and changes d_x."""
    first = R.out_shape(tuple(X.shape), [tuple(s) for s in META['specs']][:1])
    up0 = torch.randint(-2, 3, first, generator=torch.Generator().manual_seed(1)).float() / 2
    one = R.run_ref(X, PARAMS, BLOCKS, UP, False, torch.float64)
    last = R.run_ref(X, PARAMS, BLOCKS, None, False, torch.float64, ups=[torch.zeros(first), UP])
    assert sorted(last) == sorted([k for k in one if k != 'y'] + ['out0', 'out1']) and torch.equal(last['out1'], one['y'])
    only0 = R.run_ref(X, PARAMS, BLOCKS, None, False, torch.float64, ups=[up0, torch.zeros_like(UP)])
    both = R.run_ref(X, PARAMS, BLOCKS, None, False, torch.float64, ups=[up0, UP])
    for k in one:
        if k.startswith('d_'):
            assert rel_err(last[k], one[k]) <= 1e-12, k
            assert rel_err(both[k], one[k] + only0[k]) <= 1e-12, k
    assert rel_err(both['d_x'], one['d_x']) > 1e-3
    assert not bool(only0['d_1.conv1.weight'].ne(0).any()) and bool(only0['d_0.conv1.weight'].ne(0).any())
    m = R.relu_margins(X, PARAMS, BLOCKS, None, False, ups=[up0, UP])
    assert len(m) == 6 and all(lo < float('inf') for _, lo, _ in m)


def bn_desc(**kw):
    d = L.BnDesc()
    d.npos, d.C, d.training, d.relu, d.eps, d.momentum = 70, 32, 1, 0, 1e-5, 0.1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_number_and_the_batchnorm_workspace():
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9 and L.WS_CONV_WGRAD == 24 and L.WS_BN == 25
    header = open(os.path.join(HERE, '..', 'include', 'yolact_amd.h')).read()
    assert '#define YMI_ABI_VERSION 9' in header and 'YMI_WS_BN = 25' in header
    for name in ('ymi_conv_dgrad_s2_nhwc_f32', 'ymi_bn_fwd_nhwc_f32', 'ymi_bn_bwd_nhwc_f32', 'ymi_conv_dgrad_desc', 'ymi_bn_desc'):
        assert name in header
    assert C.sizeof(L.ConvDgradDesc) == 64 and C.sizeof(L.BnDesc) == 160 and C.sizeof(L.ConvWgradDesc) == 88
    ws = lambda **kw: lib.ymi_workspace_bytes(L.WS_BN, C.byref(bn_desc(**kw)))
    # chunks of max(32, ceil(npos / 1024)) positions; two [chunks, C] parts and two [C] parts
    assert ws(npos=2) == 4 * (2 * 1 * 32 + 2 * 32)
    assert ws(npos=70) == 4 * (2 * 3 * 32 + 2 * 32)
    assert ws(npos=3034, C=64) == 4 * (2 * 95 * 64 + 2 * 64)                 # 94 chunks of 32 and one of 26
    assert ws(npos=8 * 138 * 138, C=256) == 4 * (2 * 1023 * 256 + 2 * 256)    # chunks of 149 positions
    assert ws(npos=70, C=4, training=0) == 4 * (2 * 3 * 4 + 2 * 4)
    assert ws(npos=1, training=1) == EARG and ws(npos=1, training=0) > 0
    assert ws(C=30) == ESHAPE and ws(npos=0) == EARG and ws(training=2) == EARG and ws(relu=-1) == EARG


def test_argument_validation_returns_codes_without_a_gpu():
    lib = L.lib()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    aligned = C.c_void_p((ptr.value + 15) // 16 * 16)
    off = C.c_void_p(aligned.value + 4)

    def dg(**kw):
        d = L.ConvDgradDesc()
        d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = 1, 5, 7, 32, 32, 32, 3, 3, 1, 2
        d.g, d.w, d.dx = aligned, aligned, aligned
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    run = lambda **kw: lib.ymi_conv_dgrad_s2_nhwc_f32(C.byref(dg(**kw)), None)
    assert lib.ymi_conv_dgrad_s2_nhwc_f32(None, None) == ENULL
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(Cin=0), dict(Cout=0), dict(stride=1), dict(stride=0), dict(stride=3),
                dict(kh=5, kw=5, pad=2), dict(pad=0), dict(kh=1, kw=1, pad=1), dict(kh=3, kw=1)):
        assert run(**bad) == EARG, bad
    for bad in (dict(Cin=48), dict(Cout=48, ldg=48), dict(ldg=16), dict(Cout=64), dict(ldg=34), dict(g=off), dict(w=off), dict(dx=off),
                dict(B=1 << 10, H=1 << 9, W=1 << 9),                      # dx of 2^33 elements
                dict(B=1 << 8, H=1 << 9, W=1 << 9, kh=1, kw=1, pad=0, Cout=1 << 10, ldg=1 << 10)):
        assert run(**bad) == ESHAPE, bad
    for bad in (dict(g=None), dict(w=None), dict(dx=None)):
        assert run(**bad) == ENULL, bad

    def bn(**kw):
        d = bn_desc()
        for k in ('x', 'res', 'gamma', 'beta', 'running_mean', 'running_var', 'y', 'mean', 'invstd', 'dy', 'dx', 'd_res', 'dgamma',
                  'dbeta', 'ws'):
            setattr(d, k, aligned)
        d.ws_bytes = 1 << 30
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for fn in (lib.ymi_bn_fwd_nhwc_f32, lib.ymi_bn_bwd_nhwc_f32):
        assert fn(None, None) == ENULL
        for bad in (dict(npos=0), dict(C=0), dict(training=2), dict(relu=2), dict(npos=1), dict(eps=-1.0)):
            assert fn(C.byref(bn(**bad)), None) == EARG, bad
        for bad in (dict(C=30), dict(ws_bytes=16), dict(x=off), dict(ws=off), dict(npos=1 << 38)):
            assert fn(C.byref(bn(**bad)), None) == ESHAPE, bad
    fwd = lambda **kw: lib.ymi_bn_fwd_nhwc_f32(C.byref(bn(**kw)), None)
    for bad in (dict(x=None), dict(gamma=None), dict(beta=None), dict(y=None), dict(mean=None), dict(invstd=None), dict(ws=None),
                dict(training=0, running_mean=None), dict(training=0, running_var=None)):
        assert fwd(**bad) == ENULL, bad
    assert fwd(y=off) == ESHAPE and fwd(res=off) == ESHAPE
    bwd = lambda **kw: lib.ymi_bn_bwd_nhwc_f32(C.byref(bn(**kw)), None)
    for bad in (dict(dy=None), dict(ws=None), dict(relu=1, y=None), dict(x=None), dict(mean=None), dict(invstd=None), dict(gamma=None),
                dict(training=0, dx=None, d_res=None, dgamma=None, dbeta=None)):
        assert bwd(**bad) == ENULL, bad
    assert bwd(dx=off) == ESHAPE and bwd(dy=off) == ESHAPE


def test_geometry_outside_the_plain_convolution_raises_naming_it():
    assert TO.check_plain(torch.zeros(8, 32, 3, 3), 1) == (3, 1, 1) and TO.check_plain(torch.zeros(8, 64, 1, 1), 2) == (1, 0, 2)
    assert TO.check_plain(torch.zeros(8, 32, 3, 3), (2, 2)) == (3, 1, 2)
    with pytest.raises(NotImplementedError, match='5 x 5'):
        TO.check_plain(torch.zeros(8, 32, 5, 5), 1)
    with pytest.raises(NotImplementedError, match='5 x 5'):
        TO.check_plain(torch.zeros(8, 32, 5, 5), 2)
    with pytest.raises(NotImplementedError, match='stride'):
        TO.check_plain(torch.zeros(8, 32, 3, 3), 3)
    with pytest.raises(NotImplementedError, match='Cin = 3'):
        TO.check_plain(torch.zeros(64, 3, 3, 3), 2)
    # conv2d_act keeps refusing a bias-free convolution, and stride 2
    with pytest.raises(RuntimeError, match='GPU'):
        TO.conv2d_act(torch.zeros(1, 4, 4, 32), torch.zeros(8, 32, 3, 3), None, 1)
    with pytest.raises(NotImplementedError, match='stride'):
        TO.check_conv(torch.zeros(8, 32, 3, 3), 1, stride=2)


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the refusals behind require_cuda are reached without one."""
    is_cuda = True


def _gpu(t):
    return t.as_subclass(_OnGpu)


def test_python_refusals():
    x = torch.zeros(1, 4, 4, 32)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.conv2d_plain(x, torch.zeros(8, 32, 3, 3))
    with pytest.raises(RuntimeError, match='GPU'):
        TO.batch_norm_act(x, nn.BatchNorm2d(32))
    with pytest.raises(RuntimeError, match='GPU'):
        TO.bottleneck(torch.zeros(1, 4, 4, 64), M.Bottleneck(64, 32))
    with pytest.raises(NotImplementedError, match='bias = None'):
        TO.conv2d_act(_gpu(x), _gpu(torch.zeros(8, 32, 3, 3)), None, 1)
    with pytest.raises(NotImplementedError, match='momentum = None'):
        TO.batch_norm_act(_gpu(x), nn.BatchNorm2d(32, momentum=None))
    with pytest.raises(NotImplementedError, match='affine = False'):
        TO.batch_norm_act(_gpu(x), nn.BatchNorm2d(32, affine=False))
    with pytest.raises(NotImplementedError, match='track_running_stats = False'):
        TO.batch_norm_act(_gpu(x), nn.BatchNorm2d(32, track_running_stats=False))
    with pytest.raises(NotImplementedError, match='npos = 1'):
        TO.batch_norm_act(_gpu(torch.zeros(1, 1, 1, 32)), nn.BatchNorm2d(32), batch_stats=True)
    with pytest.raises(NotImplementedError, match='DCN block'):
        TO.check_bottleneck(M.Bottleneck(64, 32, use_dcn=True), 'layers.1.2')
    with pytest.raises(NotImplementedError, match='layers.1.2'):
        TO.check_bottleneck(M.Bottleneck(64, 32, use_dcn=True), 'layers.1.2')
    with pytest.raises(NotImplementedError, match='DCN block'):
        TO.bottleneck(_gpu(torch.zeros(1, 4, 4, 64)), M.Bottleneck(64, 32, use_dcn=True))
    TO.check_bottleneck(M.Bottleneck(64, 32))
    odd = M.Bottleneck(64, 32)
    odd.conv2 = nn.Conv2d(32, 32, 3, padding=2, dilation=2, bias=False)
    with pytest.raises(NotImplementedError, match='conv2'):
        TO.check_bottleneck(odd)


def test_forward_backbone_refuses_what_it_does_not_take():
    before = yolact_amd.config.cfg.copy()
    try:
        from yolact_amd.yolact import Yolact
        yolact_amd.set_cfg('yolact_resnet50_config')
        net = Yolact()
        with pytest.raises(RuntimeError, match='GPU'):
            net.forward_backbone(torch.zeros(1, 64, 9, 9))
        with pytest.raises(NotImplementedError):
            net.train()
        yolact_amd.set_cfg('yolact_plus_resnet50_config')
        with pytest.raises(NotImplementedError, match=r'backbone\.layers\.1\.\d+ is a DCN block'):
            Yolact().forward_backbone(torch.zeros(1, 64, 9, 9))
        yolact_amd.set_cfg('yolact_darknet53_config')
        with pytest.raises(NotImplementedError, match='DarkNetBackbone'):
            Yolact().forward_backbone(torch.zeros(1, 64, 9, 9))
    finally:
        yolact_amd.config.cfg.replace(before)
