"""The train-mode ResNet stem on the CPU: the oracle of tests/stem_train_ref.py is pinned to what the reference's own ResNetBackbone
object computed in both BatchNorm modes (tests/golden/stem_train.npz, tools/make_golden_stem_train.py), and the surface that needs no
GPU is checked: the ABI number and the workspace selectors, the exports, the descriptor's size, argument validation of
ymi_stem_wgrad_nhwc_f32, ymi_maxpool_fwd_nhwc_f32 and ymi_maxpool_bwd_nhwc_f32, the Python refusals, and the tie rule of PyTorch's own
max-pool that the kernels' contract names.

Golden bar: every stored output, gradient and running statistic: rel_err <= 1e-6 for the fp32 and for the fp64 oracle, the bar of
tests/test_backbone_train_host.py.
"""
import ctypes as C
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_train_ref as R  # noqa: E402
from helpers import rel_err  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

META, X, PARAMS, UP, WANT = R.load_golden()
GOLDEN_BAR = 1e-6
ENULL, EARG, ESHAPE = -3, -1, -2
MODES = (('eval', False), ('train', True))
HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ENTRIES = ('ymi_stem_wgrad_nhwc_f32', 'ymi_maxpool_fwd_nhwc_f32', 'ymi_maxpool_bwd_nhwc_f32')


def test_the_golden_case_is_the_one_the_issue_describes():
    assert tuple(X.shape) == (2, 3, 29, 23) and tuple(UP.shape) == (2, 64, 8, 6)
    assert list(PARAMS) == list(R.PARAM_NAMES) and tuple(PARAMS['conv1.weight'].shape) == (64, 3, 7, 7)
    assert sorted(WANT['eval']) == sorted(['y'] + ['d_' + n for n in R.LEAVES])
    assert sorted(WANT['train']) == sorted(['y'] + ['d_' + n for n in R.LEAVES] + ['new_' + n for n in R.STATS])
    for mode, _ in MODES:
        assert tuple(WANT[mode]['y'].shape) == (2, 64, 8, 6) and tuple(WANT[mode]['d_conv1.weight'].shape) == (64, 3, 7, 7)
        for k, v in WANT[mode].items():
            assert v.dtype == torch.float32 and bool(v.ne(0).any()), (mode, k)
    for t in [X, UP] + list(PARAMS.values()):
        assert torch.equal(t.half().float(), t)                                          # the fp16-exact grids
    for n in R.STATS:                                                                    # non-trivial running statistics, which move
        assert not torch.equal(PARAMS[n], torch.zeros_like(PARAMS[n])) and not torch.equal(PARAMS[n], torch.ones_like(PARAMS[n]))
        assert not torch.equal(WANT['train']['new_' + n], PARAMS[n])
    assert META['searched'] == 64 and 1 <= META['qualified'] <= 64 and 1 <= META['seed'] <= 64
    assert sorted(META['margins']) == ['eval', 'train'] and [m[0] for m in META['margins']['eval']] == ['relu', 'pool']
    assert os.path.getsize(os.path.join(HERE, 'golden', 'stem_train.npz')) <= 652222


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('mode', MODES, ids=['eval', 'train'])
def test_oracle_equals_the_reference(mode, dtype):
    name, train = mode
    r = R.run_ref(X, PARAMS, UP, train, dtype)
    assert sorted(k for k in r if not k.startswith('_') and (train or not k.startswith('new_'))) == sorted(WANT[name])
    for k in WANT[name]:
        e = rel_err(r[k], WANT[name][k])
        print('%s %s %s: %.3e' % (name, dtype, k, e))
        assert e <= GOLDEN_BAR, (k, e)


def test_golden_tells_a_wrong_oracle_apart():
    """The biased variance in the running update, a pool without its padding, a pool whose windows start one pixel late: not met."""
    r = R.run_ref(X, PARAMS, UP, True, torch.float64, unbiased_running=False)
    assert rel_err(r['y'], WANT['train']['y']) <= GOLDEN_BAR
    assert rel_err(r['new_bn1.running_var'], WANT['train']['new_bn1.running_var']) > 1e-4
    for name, train in MODES:
        keep = {}
        R.run_ref(X, PARAMS, UP, train, torch.float64, keep)
        a = keep['pool'][0].detach()
        assert F.max_pool2d(a, 3, 2, 0).shape != WANT[name]['y'].shape
        shifted = F.max_pool2d(a[:, :, 1:, 1:], 3, 2, 1)                   # windows that start one pixel late
        assert shifted.shape != WANT[name]['y'].shape or rel_err(shifted, WANT[name]['y']) > 1e-3


def test_margins_of_the_golden_case():
    for name, train in MODES:
        m = R.margins(X, PARAMS, UP, train)
        print('golden %s, tightest margin: %s %.3e, fp32 deviation %.3e' % ((name,) + R.tightest(m)))
        assert [t[0] for t in m] == ['relu', 'pool']
        R.assert_margins(m)
        r64, r32 = (R.run_ref(X, PARAMS, UP, train, dt) for dt in (torch.float64, torch.float32))
        assert max(rel_err(r32[k], r64[k]) for k in WANT[name]) <= 1e-6


def test_pool_gaps_sees_ties_and_allows_them_only_at_zero():
    a = torch.tensor([[0., 0., 0.], [0., 3., 1.], [0., 1., 2.5]]).view(1, 1, 3, 3)
    hit = torch.ones(1, 1, 2, 2, dtype=torch.bool)
    # windows: {0,0,0,3} gap 3; {0,0,3,1} gap 2; {0,3,0,1} gap 2; {3,1,1,2.5} gap 0.5
    assert R.pool_gaps(a, hit) == 0.5
    assert R.pool_gaps(a, torch.tensor([[[[True, False], [False, False]]]])) == 3.0
    assert R.pool_gaps(torch.zeros(1, 1, 3, 3), hit) == float('inf')            # all-zero windows: a tie at 0 is allowed
    tie = a.clone()
    tie[0, 0, 2, 2] = 3.0
    assert R.pool_gaps(tie, hit) == 0.0                                         # equal maxima away from 0
    assert R.pool_gaps(tie, torch.tensor([[[[True, True], [True, False]]]])) == 2.0
    assert R.pool_gaps(a, torch.zeros(1, 1, 2, 2, dtype=torch.bool)) == float('inf')


def test_pytorch_max_pool_sends_a_tied_gradient_to_the_first_maximum():
    """The tie rule in the kernels' contract is PyTorch's CPU one: of equal maxima the first in row-major window order."""
    x = torch.zeros(1, 1, 5, 5, requires_grad=True)
    y = F.max_pool2d(x, 3, 2, 1)
    dy = torch.arange(1., 10.).view(1, 1, 3, 3)
    (y * dy).sum().backward()
    want = torch.zeros(5, 5)
    for oy in range(3):
        for ox in range(3):
            want[max(2 * oy - 1, 0), max(2 * ox - 1, 0)] += dy[0, 0, oy, ox]       # the first real pixel of the window
    assert torch.equal(x.grad[0, 0], want)
    x = torch.tensor([[1., 2., 2.], [2., 0., 2.], [1., 2., 2.]]).view(1, 1, 3, 3).requires_grad_(True)
    F.max_pool2d(x, 3, 2, 1)[0, 0, 1, 1].backward()                            # the window rows 1 .. 2, columns 1 .. 2: 0 2 / 2 2
    assert torch.equal(x.grad[0, 0], torch.tensor([[0., 0., 0.], [0., 0., 1.], [0., 0., 0.]]))


def wg_desc(**kw):
    d = L.StemWgradDesc()
    d.B, d.H, d.W, d.Cout, d.ldg = 2, 29, 23, 64, 64
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_number_selectors_exports_and_the_descriptor():
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    assert (L.WS_CONV_WGRAD, L.WS_BN, L.WS_STEM_WGRAD) == (24, 25, 26)
    header = open(os.path.join(HERE, '..', 'include', 'yolact_amd.h')).read()
    assert '#define YMI_ABI_VERSION 9' in header
    for sel in ('YMI_WS_CONV_WGRAD = 24', 'YMI_WS_BN = 25', 'YMI_WS_STEM_WGRAD = 26'):
        assert sel in header
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    for name in NEW_ENTRIES:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in bound and bound[name][0] is C.c_int
        assert getattr(lib, name).argtypes == bound[name][1]
    assert bound['ymi_stem_wgrad_nhwc_f32'][1][0]._type_ is L.StemWgradDesc
    assert len(bound['ymi_maxpool_fwd_nhwc_f32'][1]) == 7 and len(bound['ymi_maxpool_bwd_nhwc_f32'][1]) == 8
    # the header's struct: four pointers, an int64 and six int32, in this order: 4 * 8 + 8 + 6 * 4 bytes, no padding
    body = re.search(r'typedef struct ymi_stem_wgrad_desc \{(.*?)\} ymi_stem_wgrad_desc;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert [' '.join(f.split()) for f in body.split(';') if f.strip()] == [
        'const float *x', 'const float *g', 'float *dw', 'void *ws', 'int64_t ws_bytes', 'int32_t B, H, W, Cout, ldg, _pad0']
    assert C.sizeof(L.StemWgradDesc) == 64
    assert [n for n, _ in L.StemWgradDesc._fields_] == ['x', 'g', 'dw', 'ws', 'ws_bytes', 'B', 'H', 'W', 'Cout', 'ldg', '_pad0']
    ws = lambda **kw: lib.ymi_workspace_bytes(L.WS_STEM_WGRAD, C.byref(wg_desc(**kw)))
    # P = B Ho Wo positions in chunks of 32 ceil(ceil(P / 32) / min(ceil(P / 32), ceil(512 / ceil(Cout / 64)))); [chunks][147][Cout] floats
    assert ws() == 4 * 12 * 147 * 64                                     # 360 positions: 12 chunks of 32 (the last of 8)
    assert ws(B=1, H=1, W=5, Cout=32) == 4 * 1 * 147 * 32                # 3 positions
    assert ws(B=2, H=61, W=47) == 4 * 47 * 147 * 64                      # 1488 positions: 47 chunks of 32 (the last of 16)
    assert ws(B=8, H=550, W=550) == 4 * 511 * 147 * 64                   # 605000 positions: 511 chunks of 1184 (the last of 1160)
    assert ws(B=8, H=550, W=550, Cout=96, ldg=96) == 4 * 256 * 147 * 96  # two channel groups: 256 chunks of 2368
    assert ws(Cout=48, ldg=48) == ESHAPE and ws(B=0) == EARG and ws(ldg=32) == ESHAPE
    assert lib.ymi_workspace_bytes(L.WS_STEM_WGRAD, None) == ENULL


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
    run = lambda **kw: lib.ymi_stem_wgrad_nhwc_f32(C.byref(wg(**kw)), None)
    assert lib.ymi_stem_wgrad_nhwc_f32(None, None) == ENULL
    for bad in (dict(x=None), dict(g=None), dict(dw=None), dict(ws=None)):
        assert run(**bad) == ENULL, bad
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(Cout=0), dict(Cout=-32)):
        assert run(**bad) == EARG, bad
    for bad in (dict(Cout=48, ldg=48), dict(Cout=16, ldg=16), dict(ldg=32), dict(ldg=66), dict(ws=off), dict(ws_bytes=16), dict(ws_bytes=0),
                dict(B=1 << 6, H=1 << 11, W=1 << 11),                    # x of 2^30 elements
                dict(B=1 << 5, H=1 << 10, W=1 << 10, ldg=1 << 7)):       # x of 2^27, g of 2^30 elements
        assert run(**bad) == ESHAPE, bad

    fwd = lambda x=aligned, y=aligned, B=2, H=5, W=7, Cc=32: lib.ymi_maxpool_fwd_nhwc_f32(x, y, B, H, W, Cc, None)
    bwd = lambda x=aligned, dy=aligned, dx=aligned, B=2, H=5, W=7, Cc=32: lib.ymi_maxpool_bwd_nhwc_f32(x, dy, dx, B, H, W, Cc, None)
    assert fwd(x=None) == ENULL and fwd(y=None) == ENULL
    assert bwd(x=None) == ENULL and bwd(dy=None) == ENULL and bwd(dx=None) == ENULL
    for fn in (fwd, bwd):
        for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(Cc=0)):
            assert fn(**bad) == EARG, bad
        for bad in (dict(Cc=30), dict(Cc=2), dict(x=off), dict(B=1 << 12, H=1 << 12, W=1 << 12, Cc=1 << 6)):
            assert fn(**bad) == ESHAPE, bad
    assert fwd(y=off) == ESHAPE and bwd(dy=off) == ESHAPE and bwd(dx=off) == ESHAPE


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the refusals behind require_cuda are reached without one."""
    is_cuda = True


def _gpu(t):
    return t.as_subclass(_OnGpu)


def test_python_refusals():
    x4, w = torch.zeros(1, 9, 9, 4), torch.zeros(64, 3, 7, 7)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.stem_conv(x4, w)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.stem_conv(_gpu(x4), w)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.max_pool_3x3_s2(torch.zeros(1, 9, 9, 64))
    with pytest.raises(NotImplementedError, match='stem_conv.*5 x 5'):
        TO.stem_conv(_gpu(x4), _gpu(torch.zeros(64, 3, 5, 5)))
    with pytest.raises(NotImplementedError, match='stem_conv.*stride = 1'):
        TO.stem_conv(_gpu(x4), _gpu(w), stride=1)
    with pytest.raises(NotImplementedError, match='stem_conv.*padding = 2'):
        TO.stem_conv(_gpu(x4), _gpu(w), padding=2)
    with pytest.raises(NotImplementedError, match='stem_conv.*Cin = 4'):
        TO.stem_conv(_gpu(x4), _gpu(torch.zeros(64, 4, 7, 7)))
    with pytest.raises(NotImplementedError, match='stem_conv.*a bias'):
        TO.stem_conv(_gpu(x4), _gpu(w), _gpu(torch.zeros(64)))
    with pytest.raises(NotImplementedError, match='stem_conv.*Cout = 48'):
        TO.stem_conv(_gpu(x4), _gpu(torch.zeros(48, 3, 7, 7)))
    with pytest.raises(NotImplementedError, match='stem_conv.*requires grad'):
        TO.stem_conv(_gpu(x4.clone().requires_grad_(True)), _gpu(w))
    with pytest.raises(ValueError, match='stem_conv'):
        TO.stem_conv(_gpu(torch.zeros(1, 9, 9, 3)), _gpu(w))
    with pytest.raises(NotImplementedError, match='max_pool_3x3_s2'):
        TO.max_pool_3x3_s2(_gpu(torch.zeros(1, 9, 9, 30)))
    # the plain convolution keeps refusing the stem's geometry: the stem has an entry of its own
    with pytest.raises(NotImplementedError, match='Cin = 3'):
        TO.check_plain(torch.zeros(64, 3, 3, 3), 2)
    with pytest.raises(NotImplementedError, match='7 x 7'):
        TO.check_plain(torch.zeros(64, 32, 7, 7), 2)


def test_forward_stem_and_forward_train_refuse_what_they_do_not_take():
    before = yolact_amd.config.cfg.copy()
    try:
        from yolact_amd.yolact import Yolact
        yolact_amd.set_cfg('yolact_resnet50_config')
        net = Yolact()
        with pytest.raises(RuntimeError, match='GPU'):
            net.forward_stem(torch.zeros(1, 3, 9, 9))
        with pytest.raises(RuntimeError, match='GPU'):
            net.forward_train(torch.zeros(1, 3, 9, 9))
        with pytest.raises(ValueError, match='3,H,W'):
            net.forward_stem(_gpu(torch.zeros(1, 4, 9, 9)))
        with pytest.raises(NotImplementedError):
            net.train()
        assert not net.training
        yolact_amd.set_cfg('yolact_darknet53_config')
        with pytest.raises(NotImplementedError, match='forward_stem.*DarkNetBackbone'):
            Yolact().forward_stem(torch.zeros(1, 3, 9, 9))
    finally:
        yolact_amd.config.cfg.replace(before)
