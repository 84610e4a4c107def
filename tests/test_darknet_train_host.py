"""The train-mode DarkNet53 backbone on the CPU: the oracle of tests/darknet_train_ref.py is pinned to what the reference's own
darknetconvlayer and DarkNetBlock computed in fp64 in both BatchNorm modes (tests/golden/darknet_train.npz,
tools/make_golden_darknet_train.py), and the surface that needs no GPU is checked: the exports, the header's declarations, the
bindings, the ABI number and the new workspace selector, every error code of ymi_bn_leaky_fwd_nhwc_f32, ymi_bn_leaky_bwd_nhwc_f32 and
ymi_preconv_wgrad_nhwc_f32, and the Python refusals.

Golden bar: every stored output, gradient and running statistic: rel_err <= STORED_SLACK = 1e-6 for the fp32 and for the fp64 oracle,
the bar of tests/test_backbone_train_host.py.  Two deliberately wrong oracles (the residual before the activation, slope 0.01) miss it.
"""
import ctypes as C
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import darknet_train_ref as R  # noqa: E402
from helpers import rel_err  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import modules as M  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

META, CASES = R.load_golden()
STORED_SLACK = 1e-6                                     # train_helpers.STORED_SLACK (that module needs nothing of the GPU but imports more)
ENULL, EARG, ESHAPE = -3, -1, -2
MODES = (('eval', False), ('train', True))
HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ('ymi_bn_leaky_fwd_nhwc_f32', 'ymi_bn_leaky_bwd_nhwc_f32', 'ymi_preconv_wgrad_nhwc_f32')


def test_the_golden_cases_are_the_ones_the_issue_describes():
    assert list(CASES) == ['pre', 'down', 'block'] == META['cases']
    shapes = {'pre': ((2, 3, 9, 7), (2, 32, 9, 7)), 'down': ((2, 32, 9, 7), (2, 64, 5, 4)), 'block': ((2, 64, 9, 7), (2, 64, 9, 7))}
    for case, (x, params, up, want) in CASES.items():
        assert (tuple(x.shape), tuple(up.shape)) == shapes[case]
        leaves = [n for n in params if R.is_leaf_name(n)]
        stats = [n for n in params if not R.is_leaf_name(n)]
        assert len(leaves) == (6 if case == 'block' else 3) and len(stats) == (4 if case == 'block' else 2)
        assert sorted(want['eval']) == sorted(['y', 'd_x'] + ['d_' + n for n in leaves])
        assert sorted(want['train']) == sorted(['y', 'd_x'] + ['d_' + n for n in leaves] + ['new_' + n for n in stats])
        for mode, _ in MODES:
            for k, v in want[mode].items():
                assert v.dtype == torch.float32 and bool(v.ne(0).any()), (case, mode, k)
        for t in [x, up] + list(params.values()):
            assert torch.equal(t.half().float(), t)                                      # the fp16-exact grids
        for n in stats:                                                                  # non-trivial running statistics, which move
            assert not torch.equal(want['train']['new_' + n], params[n])
        assert META['searched'] == 64 and 1 <= META['qualified'][case] <= 64 and 1 <= META['seed'][case] <= 64
    assert tuple(CASES['pre'][1]['0.weight'].shape) == (32, 3, 3, 3) and tuple(CASES['down'][1]['0.weight'].shape) == (64, 32, 3, 3)
    assert tuple(CASES['block'][1]['conv1.0.weight'].shape) == (32, 64, 1, 1)
    assert META['slope'] == 0.1 == R.SLOPE
    assert os.path.getsize(os.path.join(HERE, 'golden', 'darknet_train.npz')) <= 652222


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('mode', MODES, ids=['eval', 'train'])
@pytest.mark.parametrize('case', list(CASES))
def test_oracle_equals_the_reference(case, mode, dtype):
    name, train = mode
    x, params, up, want = CASES[case]
    r = R.run_ref(x, params, R.GOLDEN_CASES[case][0], up, train, dtype)
    assert sorted(k for k in r if not k.startswith('_') and (train or not k.startswith('new_'))) == sorted(want[name])
    for k in want[name]:
        e = rel_err(r[k], want[name][k])
        print('%s %s %s %s: %.3e' % (case, name, dtype, k, e))
        assert e <= STORED_SLACK, (k, e)


@pytest.mark.parametrize('mode', MODES, ids=['eval', 'train'])
def test_golden_tells_a_wrong_oracle_apart(mode):
    """The residual added before the activation (the bottleneck's form) and LeakyReLU(0.01): neither meets the bar."""
    name, train = mode
    x, params, up, want = CASES['block']
    net = R.GOLDEN_CASES['block'][0]
    r = R.run_ref(x, params, net, up, train, torch.float64, residual_first=True)
    assert rel_err(r['y'], want[name]['y']) > 1e-3 and rel_err(r['d_x'], want[name]['d_x']) > 1e-3
    for case in CASES:
        x, params, up, want = CASES[case]
        r = R.run_ref(x, params, R.GOLDEN_CASES[case][0], up, train, torch.float64, slope=0.01)
        assert rel_err(r['y'], want[name]['y']) > 1e-3 and rel_err(r['d_0.weight' if case != 'block' else 'd_conv1.0.weight'],
                                                                    want[name]['d_0.weight' if case != 'block' else 'd_conv1.0.weight']) > 1e-3


def test_margins_of_the_golden_cases():
    for case, (x, params, up, want) in CASES.items():
        net = R.GOLDEN_CASES[case][0]
        for name, train in MODES:
            m = R.leaky_margins(x, params, net, up, train)
            print('golden %s %s, tightest margin: %s %.3e, fp32 deviation %.3e' % ((case, name) + R.tightest(m)))
            assert len(m) == (2 if case == 'block' else 1)
            R.assert_margins(m)


def test_backbone_net_follows_the_containers_layout():
    net, taps, shapes = R.backbone_net((1, 2, 8, 8, 4))
    bb = M.DarkNetBackbone()
    want = sorted(n for n in bb.state_dict() if 'num_batches' not in n)
    have = sorted(p + s for p in shapes for s in ('0.weight', '1.weight', '1.bias', '1.running_mean', '1.running_var'))
    assert have == want
    sd = bb.state_dict()
    for p, (cin, cout, k) in shapes.items():
        assert tuple(sd[p + '0.weight'].shape) == (cout, cin, k, k), p
    assert len(taps) == 5 and len(net) == 1 + 5 + 23 and [net[t][0] for t in taps] == ['block'] * 5
    assert R.out_shapes((2, 3, 33, 29), net, shapes)[taps[-1]] == (2, 1024, 2, 1)


def wg_desc(**kw):
    d = L.PreconvWgradDesc()
    d.B, d.H, d.W, d.Cout, d.ldg = 2, 9, 7, 32, 32
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def bn_desc(**kw):
    d = L.BnDesc()
    d.npos, d.C, d.training, d.relu, d.eps, d.momentum = 70, 32, 1, 0, 1e-5, 0.1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_exports_header_bindings_abi_number_and_the_workspace():
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    assert (L.WS_STEM_WGRAD, L.WS_AUGMENT, L.WS_PRECONV_WGRAD) == (26, 27, 28)
    header = open(os.path.join(HERE, '..', 'include', 'yolact_amd.h')).read()
    assert '#define YMI_ABI_VERSION 9' in header and 'YMI_WS_PRECONV_WGRAD = 28' in header
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    for name in NEW_ENTRIES:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in bound and bound[name][0] is C.c_int
        assert getattr(lib, name).argtypes == bound[name][1]                  # the library exports it
    assert bound['ymi_preconv_wgrad_nhwc_f32'][1][0]._type_ is L.PreconvWgradDesc and len(bound['ymi_preconv_wgrad_nhwc_f32'][1]) == 2
    for name in NEW_ENTRIES[:2]:                                              # the descriptor of the plain pair, the mask, the stream
        assert bound[name][1][0]._type_ is L.BnDesc and len(bound[name][1]) == 3
    assert re.search(r'int ymi_bn_leaky_fwd_nhwc_f32\(const ymi_bn_desc \*d, uint32_t \*mask, void \*stream\);', header)
    assert re.search(r'int ymi_bn_leaky_bwd_nhwc_f32\(const ymi_bn_desc \*d, const uint32_t \*mask, void \*stream\);', header)
    assert C.sizeof(L.BnDesc) == 160                                          # the struct keeps its layout
    body = re.search(r'typedef struct ymi_preconv_wgrad_desc \{(.*?)\} ymi_preconv_wgrad_desc;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert [' '.join(f.split()) for f in body.split(';') if f.strip()] == [
        'const float *x', 'const float *g', 'float *dw', 'void *ws', 'int64_t ws_bytes', 'int32_t B, H, W, Cout, ldg, _pad0']
    assert C.sizeof(L.PreconvWgradDesc) == 64
    assert [n for n, _ in L.PreconvWgradDesc._fields_] == ['x', 'g', 'dw', 'ws', 'ws_bytes', 'B', 'H', 'W', 'Cout', 'ldg', '_pad0']
    ws = lambda **kw: lib.ymi_workspace_bytes(L.WS_PRECONV_WGRAD, C.byref(wg_desc(**kw)))
    # P = B H W positions in chunks of 32 ceil(ceil(P / 32) / min(ceil(P / 32), ceil(2048 / (Cout / 32)))); [chunks][27][Cout] floats
    assert ws() == 4 * 4 * 27 * 32                                        # 126 positions: 4 chunks of 32 (the last of 30)
    assert ws(B=1, H=1, W=1) == 4 * 1 * 27 * 32
    assert ws(B=2, H=37, W=41) == 4 * 95 * 27 * 32                        # 3034 positions: 95 chunks of 32 (the last of 26)
    assert ws(B=8, H=550, W=550) == 4 * 2044 * 27 * 32                    # 2420000 positions: 2044 chunks of 1184 (the last of 1088)
    assert ws(B=8, H=550, W=550, Cout=96, ldg=96) == 4 * 682 * 27 * 96    # three channel groups: 682 chunks of 3552
    assert ws(Cout=48, ldg=48) == ESHAPE and ws(B=0) == EARG and ws(ldg=16) == ESHAPE
    assert lib.ymi_workspace_bytes(L.WS_PRECONV_WGRAD, None) == ENULL


def test_argument_validation_returns_codes_without_a_gpu():
    lib = L.lib()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    aligned = C.c_void_p((ptr.value + 15) // 16 * 16)
    off = C.c_void_p(aligned.value + 4)

    def wg(**kw):
        d = wg_desc(x=aligned, g=aligned, dw=aligned, ws=aligned, ws_bytes=1 << 30)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    run = lambda **kw: lib.ymi_preconv_wgrad_nhwc_f32(C.byref(wg(**kw)), None)
    assert lib.ymi_preconv_wgrad_nhwc_f32(None, None) == ENULL
    for bad in (dict(x=None), dict(g=None), dict(dw=None), dict(ws=None)):
        assert run(**bad) == ENULL, bad
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(Cout=0), dict(Cout=-32)):
        assert run(**bad) == EARG, bad
    for bad in (dict(Cout=48, ldg=48), dict(Cout=16, ldg=16), dict(Cout=64), dict(ldg=34), dict(ws=off), dict(ws_bytes=16), dict(ws_bytes=0),
                dict(B=1 << 7, H=1 << 10, W=1 << 10),                    # x of 2^29 elements
                dict(B=1 << 4, H=1 << 10, W=1 << 10, ldg=1 << 5)):       # x of 2^26, g of 2^29 elements
        assert run(**bad) == ESHAPE, bad

    def bn(**kw):
        d = bn_desc()
        for k in ('x', 'res', 'gamma', 'beta', 'running_mean', 'running_var', 'y', 'mean', 'invstd', 'dy', 'dx', 'dgamma', 'dbeta', 'ws'):
            setattr(d, k, aligned)
        d.ws_bytes = 1 << 30
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    fwd = lambda mask=aligned, **kw: lib.ymi_bn_leaky_fwd_nhwc_f32(C.byref(bn(**kw)), mask, None)
    bwd = lambda mask=aligned, **kw: lib.ymi_bn_leaky_bwd_nhwc_f32(C.byref(bn(**kw)), mask, None)
    for fn in (fwd, bwd):
        # relu must be 0: the plain pair's 1 is an argument error here, like anything else
        for bad in (dict(npos=0), dict(C=0), dict(training=2), dict(relu=1), dict(relu=2), dict(relu=-1), dict(npos=1), dict(eps=-1.0)):
            assert fn(**bad) == EARG, bad
        for bad in (dict(C=30), dict(ws_bytes=16), dict(x=off), dict(ws=off), dict(npos=1 << 38)):
            assert fn(**bad) == ESHAPE, bad
        assert fn(mask=off) == ESHAPE
    assert lib.ymi_bn_leaky_fwd_nhwc_f32(None, aligned, None) == ENULL and lib.ymi_bn_leaky_bwd_nhwc_f32(None, aligned, None) == ENULL
    for bad in (dict(x=None), dict(gamma=None), dict(beta=None), dict(y=None), dict(mean=None), dict(invstd=None), dict(ws=None),
                dict(training=0, running_mean=None), dict(training=0, running_var=None)):
        assert fwd(**bad) == ENULL, bad
    assert fwd(mask=None) == ENULL                           # a residual needs the mask
    assert fwd(y=off) == ESHAPE and fwd(res=off) == ESHAPE
    for bad in (dict(dy=None), dict(ws=None), dict(x=None), dict(mean=None), dict(invstd=None), dict(gamma=None),
                dict(training=0, dx=None, dgamma=None, dbeta=None)):
        assert bwd(**bad) == ENULL, bad
    assert bwd(mask=None, y=None) == ENULL                   # the decision comes from the mask or from y
    assert bwd(d_res=aligned) == EARG                        # d_res is dy itself: no kernel writes it
    assert bwd(dx=off) == ESHAPE and bwd(dy=off) == ESHAPE


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the refusals behind require_cuda are reached without one."""
    is_cuda = True


def _gpu(t):
    return t.as_subclass(_OnGpu)


def unit(cin, cout, k, stride=1, padding=None, slope=0.1, bias=False):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2 if padding is None else padding, bias=bias),
                         nn.BatchNorm2d(cout), nn.LeakyReLU(slope, inplace=True))


def test_python_refusals_name_the_field():
    x4, w = torch.zeros(1, 9, 9, 4), torch.zeros(32, 3, 3, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.preconv(x4, w)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.preconv(_gpu(x4), w)
    with pytest.raises(NotImplementedError, match='preconv.*5 x 5'):
        TO.preconv(_gpu(x4), _gpu(torch.zeros(32, 3, 5, 5)))
    with pytest.raises(NotImplementedError, match='preconv.*stride = 2'):
        TO.preconv(_gpu(x4), _gpu(w), stride=2)
    with pytest.raises(NotImplementedError, match='preconv.*padding = 0'):
        TO.preconv(_gpu(x4), _gpu(w), padding=0)
    with pytest.raises(NotImplementedError, match='preconv.*dilation = 2'):
        TO.preconv(_gpu(x4), _gpu(w), dilation=2)
    with pytest.raises(NotImplementedError, match='preconv.*groups = 3'):
        TO.preconv(_gpu(x4), _gpu(w), groups=3)
    with pytest.raises(NotImplementedError, match='preconv.*Cin = 4'):
        TO.preconv(_gpu(x4), _gpu(torch.zeros(32, 4, 3, 3)))
    with pytest.raises(NotImplementedError, match='preconv.*a bias'):
        TO.preconv(_gpu(x4), _gpu(w), _gpu(torch.zeros(32)))
    with pytest.raises(NotImplementedError, match='preconv.*Cout = 48'):
        TO.preconv(_gpu(x4), _gpu(torch.zeros(48, 3, 3, 3)))
    with pytest.raises(NotImplementedError, match='preconv.*requires grad'):
        TO.preconv(_gpu(x4.clone().requires_grad_(True)), _gpu(w))
    with pytest.raises(ValueError, match='preconv'):
        TO.preconv(_gpu(torch.zeros(1, 9, 9, 3)), _gpu(w))

    x = torch.zeros(1, 4, 4, 32)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.batch_norm_leaky(x, nn.BatchNorm2d(32))
    with pytest.raises(RuntimeError, match='GPU'):
        TO.dark_unit(x, unit(32, 64, 3))
    with pytest.raises(RuntimeError, match='GPU'):
        TO.dark_block(torch.zeros(1, 4, 4, 64), M.DarkNetBlock(64, 32))
    with pytest.raises(NotImplementedError, match='batch_norm_leaky.*momentum = None'):
        TO.batch_norm_leaky(_gpu(x), nn.BatchNorm2d(32, momentum=None))
    with pytest.raises(NotImplementedError, match='batch_norm_leaky.*affine = False'):
        TO.batch_norm_leaky(_gpu(x), nn.BatchNorm2d(32, affine=False))
    with pytest.raises(NotImplementedError, match='batch_norm_leaky.*npos = 1'):
        TO.batch_norm_leaky(_gpu(torch.zeros(1, 1, 1, 32)), nn.BatchNorm2d(32), batch_stats=True)
    with pytest.raises(ValueError, match='batch_norm_leaky: residual'):
        TO.batch_norm_leaky(_gpu(x), nn.BatchNorm2d(32), residual=_gpu(torch.zeros(1, 4, 4, 64)))
    with pytest.raises(NotImplementedError, match='batch_norm_act.*momentum = None'):      # the shared checks keep their own name
        TO.batch_norm_act(_gpu(x), nn.BatchNorm2d(32, momentum=None))
    with pytest.raises(NotImplementedError, match='dark_unit.*negative_slope = 0.01'):
        TO.dark_unit(_gpu(x), unit(32, 64, 3, slope=0.01))
    with pytest.raises(NotImplementedError, match='dark_unit.*has a bias'):
        TO.dark_unit(_gpu(x), unit(32, 64, 3, bias=True))
    with pytest.raises(NotImplementedError, match='dark_unit.*padding = \\(0, 0\\)'):
        TO.dark_unit(_gpu(x), unit(32, 64, 3, padding=0))
    with pytest.raises(NotImplementedError, match='dark_unit.*5 x 5'):
        TO.dark_unit(_gpu(x), unit(32, 64, 5))
    with pytest.raises(NotImplementedError, match='dark_unit.*Cin = 3'):
        TO.dark_unit(_gpu(torch.zeros(1, 4, 4, 3)), unit(3, 32, 3))
    with pytest.raises(NotImplementedError, match='dark_unit.*Sequential'):
        TO.dark_unit(_gpu(x), nn.Sequential(nn.Conv2d(32, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64), nn.ReLU()))
    with pytest.raises(NotImplementedError, match='dark_block.*Bottleneck'):
        TO.dark_block(_gpu(torch.zeros(1, 4, 4, 64)), M.Bottleneck(64, 32))


def test_check_darknet_names_what_is_not_taken():
    TO.check_darknet(M.DarkNetBackbone((1, 1, 1, 1, 1)))
    TO.check_darknet(M.DarkNetBackbone())
    with pytest.raises(NotImplementedError, match='darknet.*ResNetBackbone'):
        TO.check_darknet(M.ResNetBackbone((1, 1, 1, 1)))
    bb = M.DarkNetBackbone((1, 1, 1, 1, 1))
    bb._preconv = unit(3, 32, 3, stride=2)
    with pytest.raises(NotImplementedError, match=r'backbone\._preconv\.0.*stride'):
        TO.check_darknet(bb)
    bb = M.DarkNetBackbone((1, 1, 1, 1, 1))
    bb.layers[2][0] = unit(128, 256, 3, stride=1)
    with pytest.raises(NotImplementedError, match=r'backbone\.layers\.2\.0\.0.*stride 2'):
        TO.check_darknet(bb)
    bb = M.DarkNetBackbone((1, 1, 1, 1, 1))
    bb.layers[1][1].conv2 = unit(64, 128, 3, slope=0.2)
    with pytest.raises(NotImplementedError, match=r'backbone\.layers\.1\.1\.conv2.*negative_slope = 0.2'):
        TO.check_darknet(bb)
    bb = M.DarkNetBackbone((1, 1, 1, 1, 1))
    bb.layers[3][1] = M.Bottleneck(512, 128)
    with pytest.raises(NotImplementedError, match=r'backbone\.layers\.3\.1 is a Bottleneck'):
        TO.check_darknet(bb)
    bb = M.DarkNetBackbone((1, 1, 1, 1, 1))
    bb.layers[0][1].conv1 = unit(64, 32, 3)
    with pytest.raises(NotImplementedError, match=r'backbone\.layers\.0\.1\.conv1\.0.*1 x 1'):
        TO.check_darknet(bb)


def test_the_yolact_methods_keep_refusing_a_darknet():
    before = yolact_amd.config.cfg.copy()
    try:
        from yolact_amd.yolact import Yolact
        yolact_amd.set_cfg('yolact_darknet53_config')
        net = Yolact()
        assert isinstance(net.backbone, M.DarkNetBackbone)
        TO.check_darknet(net.backbone)
        for fn, arg in ((net.forward_stem, torch.zeros(1, 3, 9, 9)), (net.forward_backbone, torch.zeros(1, 64, 9, 9)),
                        (net.forward_train, torch.zeros(1, 3, 9, 9))):
            with pytest.raises(NotImplementedError, match='DarkNetBackbone'):
                fn(_gpu(arg))
    finally:
        yolact_amd.config.cfg.replace(before)
