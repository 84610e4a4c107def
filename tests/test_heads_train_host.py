"""The train-mode heads on the CPU: the oracle of tests/heads_train_ref.py is pinned to what the reference's own Yolact computed in
train mode (tests/golden/heads_train.npz, tools/make_golden_heads_train.py), and the surface that needs no GPU is checked: the ABI
number, the workspace id, descriptor validation, refusals.

Golden bar: every stored output and every stored gradient (five leaves, twenty parameters): rel_err <= 1e-6 for the fp32 and for
the fp64 oracle, the bar of tests/test_multibox_host.py; the priors are equal.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_train_ref as H  # noqa: E402
from helpers import rel_err  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

META, OUTS, PARAMS, UPS, WANT = H.load_golden()
GOLDEN_BAR = 1e-6


def test_the_golden_case_is_the_one_the_issue_describes():
    assert [tuple(o.shape) for o in OUTS] == [(2, 32, s, s) for s in (12, 6, 3, 2, 1)]
    assert len(PARAMS) == 20 and sum(p.numel() for p in PARAMS.values()) == 83875
    assert {k: tuple(WANT[k].shape) for k in H.OUT_NAMES} == dict(loc=(2, 582, 4), conf=(2, 582, 6), mask=(2, 582, 32),
                                                                  proto=(2, 24, 24, 32), segm=(2, 5, 12, 12))
    assert sorted(WANT) == sorted(list(H.OUT_NAMES) + ['priors'] + ['d_out%d' % i for i in range(5)] + ['d_' + n for n in PARAMS])
    for t in OUTS + list(PARAMS.values()) + list(UPS.values()):
        assert torch.equal(t.half().float(), t)                            # the fp16-exact grids
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'heads_train.npz')) <= 652 * 1024
    spec, _ = H.golden_spec()
    assert H.param_names(spec) == META['params'] and {n: tuple(s) for n, s in H.param_shapes(spec, 32).items()} == \
        {n: tuple(p.shape) for n, p in PARAMS.items()}


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_oracle_equals_the_reference(dtype):
    spec, _ = H.golden_spec()
    r = H.run_ref(OUTS, PARAMS, spec, UPS, dtype)
    assert torch.equal(r['priors'], WANT['priors'])
    for k in WANT:
        if k != 'priors':
            e = rel_err(r[k], WANT[k])
            assert e <= GOLDEN_BAR, (k, e)


def test_golden_tells_a_wrong_oracle_apart():
    """Without the ReLU behind the interpolation, or with sigmoid-like saturating coefficients missing, the golden is not met."""
    spec, _ = H.golden_spec()
    wrong = dict(spec, proto_act='none')
    r = H.run_ref(OUTS, PARAMS, wrong, UPS, torch.float64)
    assert rel_err(r['proto'], WANT['proto']) > 1e-3
    wrong = dict(spec, coef_act='none')
    r = H.run_ref(OUTS, PARAMS, wrong, UPS, torch.float64)
    assert rel_err(r['mask'], WANT['mask']) > 1e-3 and rel_err(r['loc'], WANT['loc']) <= GOLDEN_BAR


def test_margins_of_the_golden_case():
    spec, _ = H.golden_spec()
    m = H.relu_margins(OUTS, PARAMS, spec, UPS)
    print('golden, tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % H.tightest(m))
    H.assert_margins(m)


def test_pack_and_unpack_round_trip():
    import numpy as np
    v = torch.randn(3, 5, generator=torch.Generator().manual_seed(0))
    planes, step = H.pack(v.numpy())
    assert (H.unpack(planes, step, (3, 5)) - v.double()).abs().max() <= step / 2 * (1 + 1e-9)
    q = np.array([0, -1, 1, -32768, 32767, 12])
    assert (H.ints_of(H.planes_of(q, 3)) == q).all()
    u = torch.tensor([-1, -0.5, 0, 0.5, 1, 1, -1])
    assert torch.equal(H.unpack5(H.pack5(u.numpy()), (7,)), u)


def test_abi_number_and_workspace_id():
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    assert L.WS_MASKIOU_HEAD == 23 and L.WS_CONV_WGRAD == 24
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'yolact_amd.h')).read()
    assert 'YMI_WS_CONV_WGRAD = 24' in header and '#define YMI_ABI_VERSION 9' in header
    d = L.ConvWgradDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = 8, 69, 69, 256, 256, 256, 3, 3, 1
    # 72 (tap, channel chunk) blocks x 15 chunks of 2560 positions: partial sums [15][2304][256] and [15][256]
    assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(d)) == 4 * 15 * (2304 * 256 + 256)
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = 2, 5, 7, 32, 12, 32, 3, 3, 1
    # 70 positions: 3 chunks of 32
    assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(d)) == 4 * 3 * (288 * 12 + 12)


def test_descriptor_validation_returns_codes_without_a_gpu():
    lib = L.lib()
    ENULL, EARG, ESHAPE = -3, -1, -2
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    aligned = C.c_void_p((ptr.value + 15) // 16 * 16)

    def wg(**kw):
        d = L.ConvWgradDesc()
        d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = 1, 2, 2, 32, 5, 32, 3, 3, 1
        d.x, d.g, d.dw, d.db, d.ws, d.ws_bytes = ptr, ptr, ptr, ptr, aligned, 1 << 30
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert lib.ymi_conv_wgrad_nhwc_f32(None, None) == ENULL
    assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, None) == ENULL
    for bad in (dict(B=0), dict(Cout=0), dict(kh=5, kw=5, pad=2), dict(kh=3, kw=3, pad=0), dict(kh=1, kw=1, pad=1), dict(kh=3, kw=1)):
        assert lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == EARG, bad
        assert lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(wg(**bad))) == EARG, bad
    for bad in (dict(Cin=48), dict(ldg=4), dict(ws_bytes=16), dict(ws=C.c_void_p(aligned.value + 4))):
        assert lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == ESHAPE, bad
    for bad in (dict(g=None), dict(ws=None), dict(dw=None, db=None), dict(x=None)):
        assert lib.ymi_conv_wgrad_nhwc_f32(C.byref(wg(**bad)), None) == ENULL, bad

    act = lib.ymi_act_bwd_f32
    assert act(ptr, None, ptr, 4, 4, 4, 4, 4, 4, L.ACT_RELU, None) == ENULL
    assert act(None, ptr, ptr, 4, 4, 4, 4, 4, 4, L.ACT_TANH, None) == ENULL          # an activation needs the output
    assert act(ptr, ptr, ptr, 4, 4, 4, 4, 4, 4, L.ACT_SIGMOID, None) == EARG
    assert act(ptr, ptr, ptr, 0, 4, 4, 4, 4, 4, L.ACT_RELU, None) == EARG
    assert act(ptr, ptr, ptr, 4, 4, 3, 4, 4, 4, L.ACT_RELU, None) == ESHAPE          # cpad < C
    assert act(ptr, ptr, ptr, 4, 4, 8, 4, 4, 4, L.ACT_RELU, None) == ESHAPE          # ldg < cpad
    assert act(ptr, ptr, ptr, 4, 4, 4, 4, 3, 4, L.ACT_NONE, None) == ESHAPE          # lddy < C

    up = lib.ymi_bilinear_bwd_nhwc_f32
    assert up(None, None, aligned, 1, 2, 2, 4, 4, 4, 0, None) == ENULL
    assert up(aligned, None, aligned, 1, 2, 2, 4, 4, 4, 1, None) == ENULL            # the ReLU mask needs the output
    assert up(aligned, aligned, aligned, 1, 2, 2, 4, 4, 4, 2, None) == EARG
    assert up(aligned, aligned, aligned, 0, 2, 2, 4, 4, 4, 0, None) == EARG
    for Ho, Wo, Cc in ((5, 4, 4), (4, 6, 4), (2, 2, 4), (4, 4, 6)):                   # other ratios, C % 4
        assert up(aligned, aligned, aligned, 1, 2, 2, Cc, Ho, Wo, 0, None) == ESHAPE
    assert up(C.c_void_p(aligned.value + 4), None, aligned, 1, 2, 2, 4, 4, 4, 0, None) == ESHAPE


def test_geometry_outside_the_kernels_raises_naming_it():
    w = torch.zeros(8, 32, 3, 3)
    assert TO.check_conv(w, 1) == (3, 1) and TO.check_conv(torch.zeros(8, 64, 1, 1), (0, 0)) == (1, 0)
    for kw, what in ((dict(stride=2), 'stride'), (dict(dilation=2), 'dilation'), (dict(groups=2), 'groups')):
        with pytest.raises(NotImplementedError, match=what):
            TO.check_conv(w, 1, **kw)
    with pytest.raises(NotImplementedError, match='5 x 5'):
        TO.check_conv(torch.zeros(8, 32, 5, 5), 2)
    with pytest.raises(NotImplementedError, match='padding'):
        TO.check_conv(w, 0)
    with pytest.raises(NotImplementedError, match='Cin = 48'):
        TO.check_conv(torch.zeros(8, 48, 3, 3), 1)


def test_cpu_tensors_raise():
    x, w, b = torch.zeros(1, 4, 4, 32), torch.zeros(8, 32, 3, 3), torch.zeros(8)
    with pytest.raises(RuntimeError, match='GPU'):
        TO.conv2d_act(x, w, b, 1, 'relu')
    with pytest.raises(RuntimeError, match='GPU'):
        TO.upsample2x(x)
    before = yolact_amd.config.cfg.copy()
    yolact_amd.set_cfg('yolact_resnet50_config')
    try:
        from yolact_amd.yolact import Yolact
        net = Yolact()
        with pytest.raises(RuntimeError, match='GPU'):
            net.forward_heads([torch.zeros(1, 256, s, s) for s in (5, 3, 2, 1, 1)])
        with pytest.raises(ValueError, match='5 prediction levels'):
            net.forward_heads([torch.zeros(1, 256, 5, 5)])
        with pytest.raises(NotImplementedError):
            net.train()
    finally:
        yolact_amd.config.cfg.replace(before)


def test_train_priors_are_cached_and_follow_cfg():
    """forward_heads builds its priors once per (level sizes, the cfg values they are made from, device) and reads cfg at every call."""
    before = yolact_amd.config.cfg.copy()
    yolact_amd.set_cfg('yolact_resnet50_config')
    try:
        from yolact_amd.yolact import Yolact
        net = Yolact()
        cfg = yolact_amd.config.cfg
        spec = H.spec_of(cfg)
        sizes = [(5, 5), (3, 3), (2, 2), (1, 1), (1, 1)]
        a = net._train_priors(sizes, cfg, torch.device('cpu'))
        assert torch.equal(a, H.priors_ref(sizes, spec)) and net._train_priors(list(sizes), cfg, torch.device('cpu')) is a
        cfg.max_size = 400
        b = net._train_priors(sizes, cfg, torch.device('cpu'))
        assert b is not a and torch.equal(b, H.priors_ref(sizes, H.spec_of(cfg))) and not torch.equal(a, b)
        cfg.backbone = cfg.backbone.copy({'use_square_anchors': False})
        c = net._train_priors(sizes, cfg, torch.device('cpu'))
        assert not torch.equal(c, b) and torch.equal(c, H.priors_ref(sizes, H.spec_of(cfg)))
        assert not torch.equal(net._train_priors(sizes[:1] + [(4, 3)] + sizes[2:], cfg, torch.device('cpu')), c)
    finally:
        yolact_amd.config.cfg.replace(before)
