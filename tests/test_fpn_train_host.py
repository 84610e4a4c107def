"""The train-mode FPN on the CPU: the oracle of tests/fpn_train_ref.py is pinned to what the reference's own FPN class computed
(tests/golden/fpn_train.npz, tools/make_golden_fpn_train.py), and the surface that needs no GPU is checked: the ABI number, the
workspace of a stride-2 weight gradient, argument validation of ymi_conv_wgrad_nhwc_f32's stride and of
ymi_bilinear_size_bwd_nhwc_f32, the Python refusals.

Golden bar: every stored output (five) and every stored gradient (three maps, sixteen parameters): rel_err <= 1e-6 for the fp32 and
for the fp64 oracle, the bar of tests/test_heads_train_host.py.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpn_train_ref as R  # noqa: E402
from helpers import rel_err  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

META, CONVOUTS, PARAMS, UPS, WANT = R.load_golden()
GOLDEN_BAR = 1e-6
ENULL, EARG, ESHAPE = -3, -1, -2


def test_the_golden_case_is_the_one_the_issue_describes():
    assert [tuple(c.shape) for c in CONVOUTS] == [(2, 64, 13, 10), (2, 96, 7, 5), (2, 128, 4, 3)]
    assert [tuple(WANT['out%d' % i].shape) for i in range(5)] == [(2, 32, 13, 10), (2, 32, 7, 5), (2, 32, 4, 3), (2, 32, 2, 2), (2, 32, 1, 1)]
    assert len(PARAMS) == 16 and list(PARAMS) == R.param_names(3, 2)
    assert {n: tuple(p.shape) for n, p in PARAMS.items()} == R.param_shapes(R.GOLDEN_IN, R.GOLDEN_NF, R.GOLDEN_DOWN)
    assert tuple(PARAMS['fpn.lat_layers.0.weight'].shape) == (32, 128, 1, 1)             # stored deepest level first
    assert sorted(WANT) == sorted(['out%d' % i for i in range(5)] + ['d_c%d' % i for i in range(3)] + ['d_' + n for n in PARAMS])
    for k, v in WANT.items():
        assert bool(v.ne(0).any()), k
    for t in CONVOUTS + list(PARAMS.values()) + UPS:
        assert torch.equal(t.half().float(), t)                                          # the fp16-exact grids
    assert all(torch.equal(p * R.PARAM_GRID, torch.round(p * R.PARAM_GRID)) for p in PARAMS.values())
    here = os.path.dirname(os.path.abspath(__file__))
    assert os.path.getsize(os.path.join(here, 'golden', 'fpn_train.npz')) <= os.path.getsize(os.path.join(here, 'golden', 'jpeg.npz')) == 652222


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_oracle_equals_the_reference(dtype):
    r = R.run_ref(CONVOUTS, PARAMS, R.GOLDEN_DOWN, UPS, dtype)
    for k in WANT:
        e = rel_err(r[k], WANT[k])
        print('%s %s: %.3e' % (dtype, k, e))
        assert e <= GOLDEN_BAR, (k, e)


def test_golden_tells_a_wrong_oracle_apart():
    """Pred layers applied in storage order to the levels finest first, or a ReLU behind the downsample layers too: not met."""
    swapped = dict(PARAMS)
    for a, b in (('fpn.pred_layers.0', 'fpn.pred_layers.2'),):
        for s in ('.weight', '.bias'):
            swapped[a + s], swapped[b + s] = PARAMS[b + s], PARAMS[a + s]
    r = R.run_ref(CONVOUTS, swapped, R.GOLDEN_DOWN, UPS, torch.float64)
    assert rel_err(r['out0'], WANT['out0']) > 1e-3 and rel_err(r['out1'], WANT['out1']) <= GOLDEN_BAR
    r = R.run_ref(CONVOUTS, PARAMS, R.GOLDEN_DOWN, UPS, torch.float64)
    assert rel_err(torch.relu(r['out3']), WANT['out3']) > 1e-3


def test_margins_of_the_golden_case():
    m = R.relu_margins(CONVOUTS, PARAMS, R.GOLDEN_DOWN, UPS)
    print('golden, tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % R.tightest(m))
    assert len(m) == 3
    R.assert_margins(m)
    r64, r32 = (R.run_ref(CONVOUTS, PARAMS, R.GOLDEN_DOWN, UPS, dt) for dt in (torch.float64, torch.float32))
    assert max(rel_err(r32[k], r64[k]) for k in WANT) <= 1e-6


def wgrad_desc(**kw):
    d = L.ConvWgradDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = 1, 2, 2, 32, 5, 32, 3, 3, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_number_and_the_workspace_of_a_stride_2_weight_gradient():
    """The chunks, hence the workspace, follow the positions of g: B * Ho * Wo with Ho = (H + 2 pad - kh) / 2 + 1."""
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9 and L.WS_CONV_WGRAD == 24
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'yolact_amd.h')).read()
    assert '#define YMI_ABI_VERSION 9' in header and 'ymi_bilinear_size_bwd_nhwc_f32' in header
    assert [n for n, _ in L.ConvWgradDesc._fields_][-2:] == ['pad', 'stride'] and C.sizeof(L.ConvWgradDesc) == 88
    ws = lambda **kw: lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(wgrad_desc(**kw)))
    small = dict(B=2, H=5, W=7, Cin=32, Cout=12, ldg=32)
    # stride 1 (the field 0 or 1): 70 positions, 3 chunks of 32; stride 2: 2 * 3 * 4 = 24 positions, one chunk
    assert ws(**small) == ws(stride=1, **small) == 4 * 3 * (288 * 12 + 12)
    assert ws(stride=2, **small) == 4 * 1 * (288 * 12 + 12)
    # the FPN's first downsample layer at B = 8: 72 (tap, channel chunk) blocks, 15 chunks wanted; 8 * 9 * 9 = 648 positions are 21
    # groups of 32 -> chunks of 64 positions -> 11 chunks (stride 1 on the same x: 2 592 positions, chunks of 192 -> 14)
    p5 = dict(B=8, H=18, W=18, Cin=256, Cout=256, ldg=256)
    assert ws(stride=2, **p5) == 4 * 11 * (2304 * 256 + 256)
    assert ws(stride=1, **p5) == 4 * 14 * (2304 * 256 + 256)
    # 1x1 / stride 2 on an even and an odd extent: (8 - 1) / 2 + 1 = 4 rows, (7 - 1) / 2 + 1 = 4 columns -> 32 positions, one chunk
    assert ws(stride=2, B=2, H=8, W=7, Cin=64, Cout=32, ldg=32, kh=1, kw=1, pad=0) == 4 * 1 * (64 * 32 + 32)
    assert ws(stride=2, B=2, H=9, W=7, Cin=64, Cout=32, ldg=32, kh=1, kw=1, pad=0) == 4 * 2 * (64 * 32 + 32)   # 40 positions


def test_argument_validation_returns_codes_without_a_gpu():
    lib = L.lib()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    aligned = C.c_void_p((ptr.value + 15) // 16 * 16)

    def wg(**kw):
        d = wgrad_desc(**kw)
        for k, v in dict(x=ptr, g=ptr, dw=ptr, db=ptr, ws=aligned, ws_bytes=1 << 30).items():
            if k not in kw:
                setattr(d, k, v)
        return d
    for bad in (dict(stride=3), dict(stride=-1), dict(stride=4), dict(stride=2, kh=5, kw=5, pad=2), dict(stride=2, kh=3, kw=3, pad=0),
                dict(stride=2, B=0)):
        assert lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == EARG, bad
        assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(wg(**bad))) == EARG, bad
    for bad in (dict(stride=2, Cin=48), dict(stride=2, ldg=4), dict(stride=2, ws_bytes=16), dict(stride=2, ws=C.c_void_p(aligned.value + 4)),
                dict(stride=2, B=1 << 12, H=1 << 10, W=1 << 10)):       # x of 2^37 elements
        assert lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == ESHAPE, bad
    for bad in (dict(stride=2, g=None), dict(stride=2, ws=None), dict(stride=2, dw=None, db=None), dict(stride=2, x=None)):
        assert lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == ENULL, bad

    up = lib.ymi_bilinear_size_bwd_nhwc_f32
    assert up(None, aligned, 1, 2, 2, 4, 3, 3, None) == ENULL
    assert up(aligned, None, 1, 2, 2, 4, 3, 3, None) == ENULL
    for B, Hi, Wi, Cc, Ho, Wo in ((0, 2, 2, 4, 3, 3), (1, 0, 2, 4, 3, 3), (1, 2, 0, 4, 3, 3), (1, 2, 2, 0, 3, 3), (1, 2, 2, 4, 0, 3),
                                  (1, 2, 2, 4, 3, -1)):
        assert up(aligned, aligned, B, Hi, Wi, Cc, Ho, Wo, None) == EARG, (B, Hi, Wi, Cc, Ho, Wo)
    for Hi, Wi, Cc, Ho, Wo in ((3, 2, 4, 2, 3), (2, 3, 4, 3, 2), (2, 2, 6, 3, 3), (2, 2, 2, 3, 3)):       # Ho < Hi, Wo < Wi, C % 4
        assert up(aligned, aligned, 1, Hi, Wi, Cc, Ho, Wo, None) == ESHAPE, (Hi, Wi, Cc, Ho, Wo)
    assert up(C.c_void_p(aligned.value + 4), aligned, 1, 2, 2, 4, 3, 3, None) == ESHAPE
    assert up(aligned, C.c_void_p(aligned.value + 8), 1, 2, 2, 4, 3, 3, None) == ESHAPE
    assert up(aligned, aligned, 1 << 10, 1 << 10, 1 << 10, 1 << 10, 1 << 10, 1 << 10, None) == ESHAPE     # 2^40 elements
    assert up(aligned, aligned, 1 << 20, 2, 2, 1 << 20, 1 << 20, 1 << 20, None) == ESHAPE                 # 2^80: no overflow either


def test_geometry_outside_the_stride_2_kernels_raises_naming_it():
    assert TO.check_down(torch.zeros(8, 32, 3, 3)) == (3, 1) and TO.check_down(torch.zeros(8, 64, 1, 1)) == (1, 0)
    with pytest.raises(NotImplementedError, match='5 x 5'):
        TO.check_down(torch.zeros(8, 32, 5, 5))
    with pytest.raises(NotImplementedError, match='3 x 1'):
        TO.check_down(torch.zeros(8, 32, 3, 1))
    with pytest.raises(NotImplementedError, match='Cin = 48'):
        TO.check_down(torch.zeros(8, 48, 3, 3))
    # the stride-1 check keeps refusing stride 2
    with pytest.raises(NotImplementedError, match='stride'):
        TO.check_conv(torch.zeros(8, 32, 3, 3), 1, stride=2)


def test_cpu_tensors_and_wrong_arguments_raise():
    x, w, b = torch.zeros(1, 4, 4, 32), torch.zeros(8, 32, 3, 3), torch.zeros(8)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.conv2d_down(x, w, b, 'relu')
    with pytest.raises(RuntimeError, match='GPU'):
        TO.upsample_add(torch.zeros(1, 2, 2, 32), x)
    before = yolact_amd.config.cfg.copy()
    yolact_amd.set_cfg('yolact_resnet50_config')
    try:
        from yolact_amd.yolact import Yolact
        net = Yolact()
        maps = lambda B=1, sizes=(5, 3, 2): [torch.zeros(B, c, s, s) for c, s in zip((512, 1024, 2048), sizes)]
        with pytest.raises(RuntimeError, match='GPU'):
            net.forward_fpn(maps())
        with pytest.raises(ValueError, match='3 lateral layers'):
            net.forward_fpn(maps()[:2])
        with pytest.raises(ValueError, match='one batch'):
            net.forward_fpn(maps()[:2] + maps(2)[2:])
        with pytest.raises(ValueError, match='larger than the level below'):
            net.forward_fpn(maps(sizes=(5, 3, 4)))
        with pytest.raises(NotImplementedError):
            net.train()
        cfg = yolact_amd.config.cfg
        cfg.fpn = cfg.fpn.copy({'pad': False})                  # read at call time
        with pytest.raises(NotImplementedError, match='fpn.pad'):
            net.forward_fpn(maps())
    finally:
        yolact_amd.config.cfg.replace(before)
