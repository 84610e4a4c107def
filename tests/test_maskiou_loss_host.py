"""The mask-IoU term 'I' on the CPU: the oracle of tests/maskiou_loss_ref.py is pinned to what the reference's own lincomb_mask_loss
and mask_iou_loss computed (tests/golden/maskiou.npz: a crowd, an instance discarded for its GT area, a border box), and the
surface that needs no GPU is checked: descriptor validation, config values, refusals.

Golden bar: 'M', 'I' and the gradients of M + I in mask, proto and the net's parameters: relative error <= 1e-6 (both sides are fp32
on the CPU), the bar of tests/test_multibox_host.py; maskiou_t and the selection equal the golden exactly.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskiou_loss_ref as IR  # noqa: E402
import multibox_ref as R  # noqa: E402
import class_loss_ref as CR  # noqa: E402
from helpers import rel_err  # noqa: E402
import yolact_amd  # noqa: E402
import yolact_amd.modules  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import maskiou_loss as MIL  # noqa: E402
from yolact_amd.layers.modules import MultiBoxLoss, MultiBoxLossPlus  # noqa: E402
import yolact_amd.layers.modules.multibox_loss as MB  # noqa: E402
import yolact_amd.layers.modules.multibox_loss_plus as MBP  # noqa: E402

META, G = IR.load_golden()
GOLDEN_BAR = 1e-6


@pytest.fixture(scope='module')
def oracle32():
    return IR.mask_and_iou_ref(IR.golden_case(G, META), torch.float32)


def test_the_golden_case_has_a_crowd_a_discarded_instance_and_a_border_box(oracle32):
    sel = G['select'].bool()
    assert META['num_crowds'] == [1, 0] and 0 < sel.sum() < sel.numel()
    assert (oracle32['inst']['box'][sel][:, 0] == 0).any()
    area = oracle32['inst']['gt'].flatten(1).sum(1)[oracle32['inst']['gt_idx'].long()]
    assert (area[~sel] <= 25).all() and (area[sel] > 25).all() and (area[~sel] > 0).all()


def test_oracle_equals_the_reference(oracle32):
    o = oracle32
    assert torch.equal(o['select'], G['select'].bool())
    assert torch.equal(o['iou_t'], G['maskiou_t'])
    assert torch.equal(o['term']['label_t'], G['label_t'].long())
    errs = {'M': rel_err(o['M'].view(1), G['M']), 'I': rel_err(o['I'].view(1), G['I']),
            'd_mask': rel_err(o['grads']['mask'], G['d_mask']), 'd_proto': rel_err(o['grads']['proto'], G['d_proto'])}
    for i, g in enumerate(o['grads']['params']):
        errs['d_param_%d' % i] = rel_err(g, G['d_param_%d' % i])
    print('  '.join('%s %.2e' % kv for kv in errs.items()))
    assert max(errs.values()) <= GOLDEN_BAR, errs


def test_golden_rejects_the_oracle_without_the_area_filter():
    o = IR.mask_and_iou_ref(IR.golden_case(G, META), torch.float32, discard_mask_area=-1)
    assert o['select'].all() and torch.equal(o['iou_t'], G['maskiou_t_all'])
    assert rel_err(o['M'].view(1), G['M']) <= GOLDEN_BAR
    assert rel_err(o['I'].view(1), G['I']) > 1e-2
    assert rel_err(o['grads']['params'][-1], G['d_param_%d' % (META['n_params'] - 1)]) > 1e-2


def test_margins_of_the_golden_case():
    case = IR.golden_case(G, META)
    m = IR.margins(lambda dtype, keep: IR.mask_and_iou_ref(case, dtype, keep=keep)['term'])
    print(m)
    IR.assert_margins(m)


def test_descriptor_validation_returns_codes_without_a_gpu():
    lib = L.lib()
    ENULL, EARG, ESHAPE = -3, -1, -2
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    off = (C.c_int32 * 2)(0, 1)
    # the net's input
    assert lib.ymi_maskiou_input_f32(None, None) == ENULL
    d = L.MaskIouInputDesc()
    d.B, d.mh, d.mw, d.K, d.N, d.G = 1, 4, 4, 32, 1, 1
    assert lib.ymi_maskiou_input_f32(C.byref(d), None) == ENULL
    assert lib.ymi_workspace_bytes(L.WS_MASKIOU_INPUT, C.byref(d)) == 4 * 32
    for name in ('proto', 'coef', 'box', 'gt', 'gt_idx', 'img_off', 'x0', 'iou_t', 'd_x0', 'd_proto', 'd_coef', 'ws'):
        setattr(d, name, ptr)
    d.img_off_host = C.cast(off, C.c_void_p)
    d.K = 16
    assert lib.ymi_maskiou_input_f32(C.byref(d), None) == ESHAPE
    d.K, d.N = 32, 0
    assert lib.ymi_maskiou_input_f32(C.byref(d), None) == EARG
    d.N = 2                                                             # the offsets end at 1
    assert lib.ymi_maskiou_input_f32(C.byref(d), None) == EARG
    assert lib.ymi_maskiou_input_bwd_f32(C.byref(d), None) == EARG
    bad = (C.c_int32 * 3)(0, 2, 1)                                      # out of order
    d.B, d.N, d.img_off_host = 2, 1, C.cast(bad, C.c_void_p)
    assert lib.ymi_maskiou_input_f32(C.byref(d), None) == EARG
    d.B, d.N, d.img_off_host, d.ws_bytes = 1, 1, C.cast(off, C.c_void_p), 4 * 32 - 1
    assert lib.ymi_maskiou_input_bwd_f32(C.byref(d), None) == ESHAPE    # a workspace that is too small
    d.mh = 1 << 13
    d.mw = 1 << 11
    assert lib.ymi_maskiou_input_f32(C.byref(d), None) == ESHAPE
    # the convolution's backward
    c = L.ConvBwdDesc()
    assert lib.ymi_conv2d_bwd_nhwc_f32(None, None) == ENULL
    assert lib.ymi_conv2d_bwd_nhwc_f32(C.byref(c), None) == EARG
    c.B, c.H, c.W, c.Cin, c.Ho, c.Wo, c.Cout, c.kh, c.kw, c.stride, c.pad, c.relu = 2, 7, 7, 4, 3, 3, 8, 3, 3, 2, 0, 1
    assert lib.ymi_conv2d_bwd_nhwc_f32(C.byref(c), None) == ENULL
    need = lib.ymi_workspace_bytes(L.WS_CONV_BWD, C.byref(c))
    assert need >= 4 * 37 * 8
    for name in ('x', 'w', 'y', 'dy', 'dx', 'dw', 'db', 'ws'):
        setattr(c, name, ptr)
    c.ws_bytes = need - 1
    assert lib.ymi_conv2d_bwd_nhwc_f32(C.byref(c), None) == ESHAPE
    c.ws_bytes, c.Ho = need, 4
    assert lib.ymi_conv2d_bwd_nhwc_f32(C.byref(c), None) == ESHAPE
    c.Ho, c.relu = 3, 2
    assert lib.ymi_conv2d_bwd_nhwc_f32(C.byref(c), None) == EARG
    c.relu, c.dy = 1, None
    assert lib.ymi_conv2d_bwd_nhwc_f32(C.byref(c), None) == ENULL
    assert lib.ymi_workspace_bytes(L.WS_CONV_BWD, None) == ENULL
    wide = L.ConvBwdDesc()                                              # 16385 x 16 tiles of [K + 1, Cout]: over the grid's limit
    wide.B, wide.H, wide.W, wide.Cin, wide.Ho, wide.Wo, wide.Cout, wide.kh, wide.kw, wide.stride = 1, 1, 1, 1 << 20, 1, 1, 1024, 1, 1, 1
    assert lib.ymi_workspace_bytes(L.WS_CONV_BWD, C.byref(wide)) == ESHAPE
    # the pool's backward and the head
    assert lib.ymi_global_maxpool_bwd_nhwc_f32(None, ptr, ptr, 1, 1, 1, None) == ENULL
    assert lib.ymi_global_maxpool_bwd_nhwc_f32(ptr, ptr, ptr, 1, 0, 1, None) == EARG
    h = L.MaskIouHeadDesc()
    assert lib.ymi_maskiou_head_f32(C.byref(h), None) == EARG
    h.N, h.C = 3, 80
    assert lib.ymi_maskiou_head_f32(C.byref(h), None) == ENULL
    assert lib.ymi_workspace_bytes(L.WS_MASKIOU_HEAD, C.byref(h)) == 16
    for name in ('pool', 'iou_t', 'label', 'loss', 'ws'):
        setattr(h, name, ptr)
    h.ws_bytes = 8
    assert lib.ymi_maskiou_head_f32(C.byref(h), None) == ESHAPE
    assert lib.ymi_abi_version() == 9 and (L.WS_MASKIOU_INPUT, L.WS_CONV_BWD, L.WS_MASKIOU_HEAD) == (21, 22, 23)


def test_the_new_config_fields_carry_the_reference_values():
    """data/config.py:642-647, 787-791."""
    for name, cfg in yolact_amd.CONFIGS.items():
        plus = 'plus' in name
        assert cfg.maskiou_alpha == (25 if plus else 1.0), name
        assert cfg.discard_mask_area == (25 if plus else -1), name
        assert cfg.maskious_to_train == -1, name
        assert bool(cfg.use_maskiou) == plus, name
        if plus:
            MB.check_switches(cfg, allow_maskiou=True)
            MIL.check_switches(cfg)
            with pytest.raises(NotImplementedError, match='use_maskiou'):
                MB.check_switches(cfg)


def test_maskious_to_train_raises_naming_the_field(monkeypatch):
    cfg = yolact_amd.CONFIGS['yolact_plus_base_config'].copy({'maskious_to_train': 5})
    with pytest.raises(NotImplementedError, match='maskious_to_train'):
        MIL.check_switches(cfg)
    for mod in (MB, MBP, MIL):
        monkeypatch.setattr(mod, 'active_cfg', lambda: cfg)
    meta, g = CR.load_golden()
    preds, targets, masks, ncs = R.golden_forward(g, meta)
    with pytest.raises(NotImplementedError, match='maskious_to_train'):
        MultiBoxLossPlus(81, 0.5, 0.4, 3)(None, preds, targets, masks, ncs)


def test_cpu_tensors_raise(monkeypatch):
    cfg = yolact_amd.CONFIGS['yolact_plus_base_config'].copy()
    for mod in (MB, MBP, MIL):
        monkeypatch.setattr(mod, 'active_cfg', lambda: cfg)
    net = yolact_amd.modules.FastMaskIoUNet(cfg.maskiou_net, 81)
    with pytest.raises(RuntimeError, match='GPU'):
        net(torch.zeros(1, 1, 63, 63))
    with pytest.raises(RuntimeError, match='GPU'):
        MIL.mask_iou_loss(net, [torch.zeros(2, 1, 63, 63), torch.zeros(2), torch.zeros(2, dtype=torch.long)])
    case = IR.golden_case(G, META)
    s = IR.instances_ref(case, torch.float32)
    with pytest.raises(RuntimeError, match='GPU'):
        MIL.lincomb_mask_loss_maskiou(s['pos'], s['idx_t'], s['mask'], s['proto'], s['obj_masks'], s['gt_box_t'], s['labels'])
    meta, g = CR.load_golden()
    preds, targets, masks, ncs = R.golden_forward(g, meta)
    with pytest.raises(RuntimeError):
        MultiBoxLossPlus(81, 0.5, 0.4, 3)(net, preds, targets, masks, ncs)
    with pytest.raises(NotImplementedError, match='use_maskiou'):
        MultiBoxLoss(81, 0.5, 0.4, 3)(net, preds, targets, masks, ncs)
