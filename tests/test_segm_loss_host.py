"""The semantic segmentation loss 'S' on the CPU: tests/segm_loss_ref.py is pinned to what the reference's own
semantic_segmentation_loss computed (tests/golden/multibox.npz), shown to tell the sum-instead-of-OR variant apart, and the C ABI /
Python surface of ymi_segm_loss_f32 is checked as far as that goes without a GPU.

Golden bar: 'S' and d S / d segm relative error <= 1e-6 (both sides are fp32 on the CPU).
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_loss_ref as CR  # noqa: E402
import segm_loss_ref as R  # noqa: E402
import yolact_amd.layers.segm_loss as SL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META, G = CR.load_golden()
GOLDEN_BAR = 1e-6


def golden_inputs():
    """The forward case's segm and its non-crowd masks and labels, prepared as the Python layer prepares them."""
    segm = G['fwd_segm'].float()
    masks, labels = [], []
    for b, nc in enumerate(META['num_crowds']):
        t, m = G['fwd_targets_%d' % b], G['fwd_masks_%d' % b].float()
        n = t.size(0) - nc
        masks.append(m[:n])
        labels.append(t[:n, 4].long())
    gt, label, off = SL.downsample_targets(masks, labels, segm.size(2), segm.size(3), 'cpu')
    return segm, gt, label, off


def test_ref_equals_the_reference():
    segm, gt, label, off = golden_inputs()
    assert gt.dtype == torch.uint8 and gt.any() and off == [0, 3, 5]
    loss, d = R.segm_ref(segm, gt, label, off, META['semantic_segmentation_alpha'])
    errs = (CR.rel_err(loss.view(1), G['segm_S']), CR.rel_err(d, G['segm_d_segm']))
    print('S %.3e d_segm %.3e' % errs)
    assert max(errs) <= GOLDEN_BAR, errs


def overlap_inputs():
    """The `segm2` case: two overlapping objects of class 19 in image 0, recorded from the reference's own call."""
    segm = G['segm2_segm'].float()
    masks = [G['segm2_masks_%d' % b].float() for b in range(2)]
    labels = [G['segm2_labels_%d' % b].long() for b in range(2)]
    gt, label, off = SL.downsample_targets(masks, labels, segm.size(2), segm.size(3), 'cpu')
    return segm, gt, label, off


def test_two_overlapping_objects_of_one_class_are_ored_as_the_reference_does():
    segm, gt, label, off = overlap_inputs()
    assert off == [0, 3, 4] and label[0] == label[1] == 19 and label[2] != 19
    both, a_only, b_only = gt[0] & gt[1], gt[0] & ~gt[1] & 1, gt[1] & ~gt[0] & 1
    assert both.any() and a_only.any() and b_only.any()               # they overlap, and each has pixels of its own
    loss, d = R.segm_ref(segm, gt, label, off, META['semantic_segmentation_alpha'])
    errs = (CR.rel_err(loss.view(1), G['segm2_S']), CR.rel_err(d, G['segm2_d_segm']))
    print('segm2: S %.3e d_segm %.3e' % errs)
    assert max(errs) <= GOLDEN_BAR, errs


def test_golden_rejects_sum_instead_of_or_for_two_objects_of_one_class():
    segm, gt, label, off = overlap_inputs()
    loss, d = R.segm_ref(segm, gt, label, off, META['semantic_segmentation_alpha'], combine='sum')
    assert CR.rel_err(loss.view(1), G['segm2_S']) > 10 * GOLDEN_BAR and CR.rel_err(d, G['segm2_d_segm']) > 0.1   # one pixel of 20 in one channel of 80
    # ... and only through the overlap: without it the two variants agree
    segm1, gt1, label1, off1 = golden_inputs()
    assert torch.equal(R.segm_ref(segm1, gt1, label1, off1, combine='sum')[0], R.segm_ref(segm1, gt1, label1, off1)[0])


def test_entries_are_exported_and_bound_at_abi_9():
    from yolact_amd import _lib as L
    lib = L.lib()
    assert lib.ymi_abi_version() == 9
    assert 'ymi_segm_loss_f32' in {name for name, _, _ in L.SYMBOLS}
    assert lib.ymi_segm_loss_f32.argtypes[0] == ctypes.POINTER(L.SegmLossDesc)
    assert L.WS_SEGM_LOSS == 20


def test_descriptor_matches_c_compiler(tmp_path):
    from yolact_amd import _lib as L
    fields = [f for f, _ in L.SegmLossDesc._fields_]
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%d"%s);'
                   % (os.path.join(ROOT, 'include', 'yolact_amd.h'), ',sizeof(ymi_segm_loss_desc),(int)YMI_WS_SEGM_LOSS')
                   + ''.join('printf(" %%zu",offsetof(ymi_segm_loss_desc,%s));' % f for f in fields) + 'return 0;}')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = L.SegmLossDesc
    assert got == [ctypes.sizeof(D), 20] + [getattr(D, f).offset for f in fields]
    assert ctypes.sizeof(D) == 8 * 8 + 6 * 4


POINTERS = ('segm', 'gt', 'label', 'gt_off', 'loss', 'd_segm', 'ws')


def _desc(off_vals=(0, 2, 5), **over):
    """Every device pointer set to an address nothing may touch: a launch would fault, a validation error returns."""
    from yolact_amd import _lib as L
    d = L.SegmLossDesc()
    for f in POINTERS:
        setattr(d, f, 16)
    keep = (ctypes.c_int32 * len(off_vals))(*off_vals)
    d.gt_off_host = ctypes.cast(keep, ctypes.c_void_p)
    d.B, d.K, d.mh, d.mw, d.G, d.alpha = 2, 80, 13, 11, 5, 1.0
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


BAD = [({f: None}, -3) for f in ('segm', 'gt', 'label', 'gt_off', 'gt_off_host', 'loss', 'ws')] + [
    ({'B': 0}, -1), ({'K': 0}, -1), ({'K': 129}, -1), ({'mh': 0}, -1), ({'mw': 0}, -1), ({'G': -1}, -1),
    ({'off_vals': (1, 2, 5)}, -1), ({'off_vals': (0, 2, 4)}, -1), ({'off_vals': (0, 6, 5)}, -1),
    ({'B': 2, 'K': 128, 'mh': 4096, 'mw': 2048}, -2),                   # B K mh mw = 2^31
    ({'B': 1, 'K': 1, 'mh': (1 << 31) - 255, 'mw': 1}, -2),             # one pixel more than 2^31 - a tile: a pixel index would pass int
    ({'segm': 20}, -2), ({'d_segm': 8}, -2), ({'ws': 24}, -2),
]


@pytest.mark.parametrize('over,code', BAD, ids=lambda v: '-'.join('%s=%s' % kv for kv in v.items()) if isinstance(v, dict) else str(v))
def test_rejects_bad_descriptors_without_a_gpu(over, code):
    from yolact_amd import _lib as L
    d, keep = _desc(**over)
    assert L.lib().ymi_segm_loss_f32(ctypes.byref(d), None) == code
    assert L.lib().ymi_segm_loss_f32(None, None) == -3


def test_workspace_sizes():
    from yolact_amd import _lib as L
    def ws(**o):
        d, keep = _desc(**o)
        return L.lib().ymi_workspace_bytes(L.WS_SEGM_LOSS, ctypes.byref(d))
    assert ws(B=8, mh=69, mw=69) == (4 * 8 * ((69 * 69 + 255) // 256) + 15) // 16 * 16
    assert ws(B=3, mh=13, mw=11) == 16 and ws(K=0) == -1 and ws(B=0) == -1
    assert ws(B=1, K=1, mh=(1 << 31) - 256, mw=1) == 4 * 8388607 + 4 and ws(B=1, K=1, mh=(1 << 31) - 255, mw=1) == -2
    assert L.lib().ymi_workspace_bytes(L.WS_SEGM_LOSS, None) == -3


def test_every_shipped_config_carries_the_reference_values():
    """data/config.py:545 and use_semantic_segmentation_loss of every shipped config."""
    import yolact_amd
    for name, cfg in yolact_amd.CONFIGS.items():
        assert cfg.semantic_segmentation_alpha == 1 and cfg.use_semantic_segmentation_loss is True, name


def test_cpu_tensors_raise(monkeypatch):
    import yolact_amd
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    monkeypatch.setattr(SL, 'active_cfg', lambda: cfg)
    segm, gt, label, off = golden_inputs()
    with pytest.raises(RuntimeError):
        SL.segm_loss(segm.clone().requires_grad_(True), gt, label, off, 1.0)
    with pytest.raises(RuntimeError):
        SL.semantic_segmentation_loss(segm, [G['fwd_masks_0'].float()[:3], G['fwd_masks_1'].float()],
                                      [G['fwd_targets_0'][:3, 4].long(), G['fwd_targets_1'][:, 4].long()])
    assert issubclass(SL.LC.LossFunction, torch.autograd.Function)
