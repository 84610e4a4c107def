"""The lincomb mask loss, on the CPU: the fp64 formula of tests/mask_loss_ref.py is pinned to what the reference's own
MultiBoxLoss.lincomb_mask_loss computed (tests/golden/mask_loss.npz, written by tools/make_golden_mask_loss.py), and the C ABI /
Python surface of ymi_mask_loss_f32 is checked as far as that goes without a GPU.

Golden bar: loss, d_proto and d_coef (as d mask_data) relative error <= 2e-6.  The reference's fp32 CPU result sits 1.0e-7 to
1.9e-7 from an fp64 statement at 12x10, 35x37 and 138x138; the bar leaves an order of magnitude for the fp32 summation order of
another torch build.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mask_loss_ref import mask_loss_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mask_loss.npz')
GOLDEN_BAR = 2e-6
_Z = np.load(GOLDEN)
META = json.loads(bytes(_Z['meta']).decode())


def _err(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def golden_case(name):
    """-> (case meta, dict of torch tensors; 'masks' a list of float [n_gt,H,W])."""
    m = next(c for c in META['cases'] if c['name'] == name)
    t = {k: torch.from_numpy(_Z['%s_%s' % (name, k)]) for k in ('proto', 'mask_data', 'pos', 'idx_t', 'gt_box_t', 'M', 'd_proto',
                                                                 'd_mask_data')}
    t['masks'] = [torch.from_numpy(_Z['%s_masks_%d' % (name, b)]).float() for b in range(len(m['ns']))]
    t['select'] = {b: torch.from_numpy(_Z['%s_select_%d' % (name, b)]) for b in m['over_cap']}
    return m, t


@pytest.mark.parametrize('name', [c['name'] for c in META['cases']])
def test_formula_equals_the_reference(name):
    from yolact_amd.layers.mask_loss import gather_instances
    m, t = golden_case(name)
    proto = t['proto'].double().requires_grad_(True)
    mask_data = t['mask_data'].double().requires_grad_(True)
    torch.manual_seed(META['torch_seed'])
    coef, box, gt, gt_idx, img_off, weight, selects = gather_instances(t['pos'], t['idx_t'], mask_data, t['masks'], t['gt_box_t'],
                                                                       m['mh'], m['mw'], META['masks_to_train'])
    assert [int(v) for v in img_off] == [0] + list(np.cumsum([min(n, META['masks_to_train']) for n in m['ns']]))
    for b, sel in enumerate(selects):
        assert (sel is not None) == (b in t['select'])
        if sel is not None:
            assert torch.equal(sel, t['select'][b])
            assert weight[int(img_off[b])].item() == np.float32(m['ns'][b] / META['masks_to_train'])
    loss, _ = mask_loss_ref(proto, coef, box, gt, gt_idx, img_off, weight, True, True, META['mask_alpha'])
    dp, dm = torch.autograd.grad(loss, [proto, mask_data])
    errs = (_err(loss.detach().view(1), t['M'].double().view(1)), _err(dp, t['d_proto'].double()),
            _err(dm, t['d_mask_data'].double()))
    print('%s: loss %.3e d_proto %.3e d_coef %.3e' % ((name,) + errs))
    assert max(errs) <= GOLDEN_BAR, errs


# ---- the C ABI and the Python surface, without a GPU -----------------------------------------------------------------------

def test_entry_is_exported_and_bound_at_abi_9():
    from yolact_amd import _lib as L
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    assert any(name == 'ymi_mask_loss_f32' for name, _, _ in L.SYMBOLS)
    assert lib.ymi_mask_loss_f32.argtypes[0] == ctypes.POINTER(L.MaskLossDesc)
    assert L.WS_MASK_LOSS == 16


def test_descriptor_matches_c_compiler(tmp_path):
    from yolact_amd import _lib as L
    fields = ('coef', 'gt', 'weight', 'loss', 'ws', 'B', 'K', 'G', 'roi_norm', 'alpha')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%d"%s);'
                   % (os.path.join(ROOT, 'include', 'yolact_amd.h'), ',sizeof(ymi_mask_loss_desc),(int)YMI_WS_MASK_LOSS')
                   + ''.join('printf(" %%zu",offsetof(ymi_mask_loss_desc,%s));' % f for f in fields) + 'return 0;}')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = L.MaskLossDesc
    assert got == [ctypes.sizeof(D), L.WS_MASK_LOSS] + [getattr(D, f).offset for f in fields]
    assert ctypes.sizeof(D) == 12 * 8 + 10 * 4


POINTERS = ('proto', 'coef', 'box', 'gt', 'gt_idx', 'img_off', 'weight', 'loss', 'loss_inst', 'd_proto', 'd_coef', 'ws')


def _desc(**over):
    """Every pointer set to an address nothing may touch: a launch would fault, a validation error returns."""
    from yolact_amd import _lib as L
    d = L.MaskLossDesc()
    for f in POINTERS:
        setattr(d, f, 16)
    d.B, d.mh, d.mw, d.K, d.N, d.G, d.crop, d.roi_norm, d.alpha = 2, 12, 10, 32, 5, 3, 1, 1, 6.125
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize('over,code', [
    ({'K': 16}, -2), ({'K': 64}, -2), ({'K': 0}, -2),
    ({'B': 0}, -1), ({'mh': 0}, -1), ({'mw': -1}, -1), ({'N': -1}, -1), ({'G': 0}, -1), ({'crop': 2}, -1), ({'roi_norm': -1}, -1),
    ({'proto': 20}, -2), ({'d_proto': 8}, -2),
    ({'proto': None}, -3), ({'img_off': None}, -3), ({'loss': None}, -3), ({'coef': None}, -3), ({'box': None}, -3),
    ({'gt': None}, -3), ({'gt_idx': None}, -3), ({'weight': None}, -3), ({'ws': None}, -3),
])
def test_rejects_bad_descriptors_without_a_gpu(over, code):
    from yolact_amd import _lib as L
    assert L.lib().ymi_mask_loss_f32(ctypes.byref(_desc(**over)), None) == code
    assert L.lib().ymi_mask_loss_f32(None, None) == -3


def test_workspace_is_positive_and_grows_with_n():
    from yolact_amd import _lib as L
    ws = lambda **o: L.lib().ymi_workspace_bytes(L.WS_MASK_LOSS, ctypes.byref(_desc(**o)))
    sizes = [ws(N=n, mh=138, mw=138) for n in (0, 1, 100, 800)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[3] >= 4 * 800 * 33 * ((138 * 138 + 255) // 256)          # a d_coef row and an L_j per 256-pixel tile and instance
    assert ws(K=16) == -2 and ws(B=0) == -1
    assert L.lib().ymi_workspace_bytes(L.WS_MASK_LOSS, None) == -3


def _wrapper_args():
    _, t = golden_case('tile12x10')
    return t['pos'], t['idx_t'], t['mask_data'], t['proto'], t['masks'], t['gt_box_t']


SWITCHES = [('mask_proto_crop_with_pred_box', True), ('mask_proto_remove_empty_masks', True), ('mask_proto_reweight_mask_loss', True),
            ('mask_proto_normalize_mask_loss_by_sqrt_area', True), ('mask_proto_double_loss', True),
            ('mask_proto_coeff_diversity_loss', True), ('mask_proto_binarize_downsampled_gt', False),
            ('use_mask_scoring', True),
            ('mask_proto_mask_activation', 'relu'), ('mask_proto_mask_activation', torch.tanh)]


@pytest.mark.parametrize('field,value', SWITCHES, ids=lambda v: v if isinstance(v, str) else getattr(v, '__name__', str(v)))
def test_every_unsupported_switch_names_its_field(monkeypatch, field, value):
    import yolact_amd
    from yolact_amd.layers import mask_loss as ML
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy({field: value})
    monkeypatch.setattr(ML, 'active_cfg', lambda: cfg)
    with pytest.raises(NotImplementedError, match=field):
        ML.lincomb_mask_loss(*_wrapper_args())


def test_every_shipped_config_carries_the_reference_values():
    """data/config.py: masks_to_train is 100 (coco_base_config:459) except yolact_im700_config (:718, 300); mask_alpha 6.125 (:689)."""
    import yolact_amd
    from yolact_amd.layers.mask_loss import check_switches
    assert {'yolact_base_config', 'yolact_plus_base_config', 'yolact_im700_config'} <= set(yolact_amd.CONFIGS)
    for name, cfg in yolact_amd.CONFIGS.items():
        check_switches(cfg)
        assert cfg.mask_proto_crop is True and cfg.mask_proto_normalize_emulate_roi_pooling is True, name
        assert cfg.masks_to_train == (300 if name == 'yolact_im700_config' else 100), name
        assert cfg.mask_alpha == 6.125, name


def test_cpu_tensors_raise(monkeypatch):
    import yolact_amd
    from yolact_amd.layers import mask_loss as ML
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    monkeypatch.setattr(ML, 'active_cfg', lambda: cfg)
    with pytest.raises(RuntimeError):
        ML.lincomb_mask_loss(*_wrapper_args())
    m, t = golden_case('tile12x10')
    coef, box, gt, gt_idx, img_off, weight, _ = ML.gather_instances(t['pos'], t['idx_t'], t['mask_data'], t['masks'], t['gt_box_t'],
                                                                    m['mh'], m['mw'], 100)
    with pytest.raises(RuntimeError):
        ML.mask_loss(t['proto'].requires_grad_(True), coef, box, gt, gt_idx, img_off, weight)
    assert issubclass(ML.LC.LossFunction, torch.autograd.Function)
