"""The semantic segmentation loss 'S' on the GPU (csrc/segm_loss.hip, ymi_segm_loss_f32, yolact_amd/layers/segm_loss.py) against
tests/segm_loss_ref.py, which tests/test_segm_loss_host.py pins to the reference's own results.

Bar: 'S' and d_segm rel_err against the fp64 oracle <= max(4 * rel_err(the same in fp32 on the CPU, fp64), EXACT_BAR = 8e-6), the
project's bar (tests/test_gpu_match.py).  Two runs give the same bits.  The largest rel_err per case is printed at the end of the
module (the table of DESIGN.md 5.4).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_loss_ref as CR  # noqa: E402
import segm_loss_ref as R  # noqa: E402
from helpers import same_bits  # noqa: E402
import yolact_amd  # noqa: E402
import yolact_amd.layers.segm_loss as SL  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT_BAR = 8e-6
_MAX = {}


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nsegmentation loss: rel_err against the fp64 oracle (bar)')
    for case in _MAX:
        print('  %-14s ' % case + '  '.join('%s %.2e (%.1e)' % (n, e, b) for n, (e, b) in _MAX[case].items()))


def boxes_as_masks(g, n, mh, mw):
    """n random rectangles as uint8 [n,mh,mw]."""
    m = torch.zeros(n, mh, mw, dtype=torch.uint8)
    for j in range(n):
        y0, x0 = int(torch.randint(0, mh - 1, (1,), generator=g)), int(torch.randint(0, mw - 1, (1,), generator=g))
        y1, x1 = int(torch.randint(y0 + 1, mh + 1, (1,), generator=g)), int(torch.randint(x0 + 1, mw + 1, (1,), generator=g))
        m[j, y0:y1, x0:x1] = 1
    return m


def small_case():
    """13x11, K = 80, B = 3.  Image 0: labels on the bitset word edges and two overlapping objects of class 31; image 1: no
    object; image 2: 70 objects, more than one LDS chunk of 64.  Some logits are +-100."""
    g = torch.Generator().manual_seed(60)
    mh, mw, K = 13, 11, 80
    l0 = [0, 31, 32, 63, 64, 79, 31]
    gt0 = boxes_as_masks(g, len(l0), mh, mw)
    gt0[1] = 0; gt0[1, 2:9, 1:7] = 1
    gt0[6] = 0; gt0[6, 5:12, 4:10] = 1                                  # overlaps object 1, the same class
    assert (gt0[1] & gt0[6]).any()
    gt2 = boxes_as_masks(g, 70, mh, mw)
    l2 = torch.randint(0, K, (70,), generator=g)
    l2[64:] = torch.tensor([79, 0, 33, 64, 5, 70])                       # the second chunk sets bits of its own
    gt = torch.cat([gt0, gt2])
    label = torch.cat([torch.tensor(l0), l2])
    off = [0, 7, 7, 77]
    segm = torch.randn(3, K, mh, mw, generator=g) * 2
    flat = segm.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:200]
    flat[idx[:100]], flat[idx[100:]] = 100.0, -100.0
    return segm, gt, label, off


def check(name, segm, gt, label, off, alpha=1.0):
    want, dwant = R.segm_ref(segm.double(), gt, label, off, alpha)
    cpu, dcpu = R.segm_ref(segm, gt, label, off, alpha)
    loss, d = SL.segm_terms(segm.to(DEV), gt.to(DEV), label.to(DEV), off, alpha)
    torch.cuda.synchronize()
    loss, d = loss.cpu(), d.cpu()
    errs = {'S': (CR.rel_err(loss, want.view(1)), max(4 * CR.rel_err(cpu.view(1), want.view(1)), EXACT_BAR)),
            'd_segm': (CR.rel_err(d, dwant), max(4 * CR.rel_err(dcpu, dwant), EXACT_BAR))}
    _MAX[name] = errs
    for k, (e, bar) in errs.items():
        print('%s %s: rel_err %.3e (bar %.3e)' % (name, k, e, bar))
        assert e <= bar, (name, k, e, bar)
    assert torch.isfinite(loss).all() and torch.isfinite(d).all()
    return loss, d


def test_word_edges_overlap_an_empty_image_and_70_objects():
    segm, gt, label, off = small_case()
    loss, d = check('13x11', segm, gt, label, off, 1.0)
    t = R.segm_targets(gt, label, off, 3, 80, torch.float32)
    assert t.max() == 1 and not t[1].any()
    for c in (0, 31, 32, 63, 64, 79):                                   # the gradient's sign shows the target bit of every word edge
        on = t[0, c].bool()
        assert on.any() and (d[0, c][on] <= 0).all() and (d[0, c][~on] >= 0).all()
    again = SL.segm_terms(segm.to(DEV), gt.to(DEV), label.to(DEV), off, 1.0)
    same_bits(again[0], loss, 'S')
    same_bits(again[1], d, 'd_segm')


def test_a_batch_without_any_object():
    g = torch.Generator().manual_seed(61)
    segm = torch.randn(2, 80, 13, 11, generator=g)
    check('no_objects', segm, torch.zeros(0, 13, 11, dtype=torch.uint8), torch.zeros(0, dtype=torch.long), [0, 0, 0], 0.5)


def test_a_label_out_of_range_gives_nan():
    segm, gt, label, off = small_case()
    label = label.clone()
    label[3] = 80
    loss, d = SL.segm_terms(segm.to(DEV), gt.to(DEV), label.to(DEV), off, 1.0)
    assert torch.isnan(loss).all()


def test_backward_is_d_segm_times_the_upstream_scalar_and_the_reference_arguments(monkeypatch):
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    monkeypatch.setattr(SL, 'active_cfg', lambda: cfg)
    segm, gt, label, off = small_case()
    loss0, d0 = SL.segm_terms(segm.to(DEV), gt.to(DEV), label.to(DEV), off, 1.0)
    x = segm.to(DEV).requires_grad_(True)
    loss = SL.segm_loss(x, gt.to(DEV), label.to(DEV), off, 1.0)
    assert loss.dim() == 0 and torch.equal(loss.detach().view(1).view(torch.int32), loss0.view(torch.int32))
    (gx,) = torch.autograd.grad(loss * 0.37, [x])
    assert torch.equal(gx, d0 * 0.37)
    # the reference's arguments: full-size float masks per image, downsampled and binarised by the Python layer
    g = torch.Generator().manual_seed(62)
    masks = [boxes_as_masks(g, n, 52, 44).float().to(DEV) for n in (3, 0, 2)]
    labels = [torch.randint(0, 80, (n,), generator=g).to(DEV) for n in (3, 0, 2)]
    got = SL.semantic_segmentation_loss(segm.to(DEV), masks, labels)
    sgt, slabel, soff = SL.downsample_targets([m.cpu() for m in masks], [l.cpu() for l in labels], 13, 11, 'cpu')
    want = R.segm_ref(segm.double(), sgt, slabel, soff, 1.0)[0]
    assert soff == [0, 3, 3, 5] and CR.rel_err(got.detach().cpu().view(1), want.view(1)) <= EXACT_BAR


def test_full_size_8x80x69x69():
    g = torch.Generator().manual_seed(63)
    B, K, mh, mw = 8, 80, 69, 69
    ns = [10, 1, 0, 25, 7, 12, 3, 9]
    gt = torch.cat([boxes_as_masks(g, n, mh, mw) for n in ns])
    label = torch.randint(0, K, (sum(ns),), generator=g)
    off = [0]
    for n in ns:
        off.append(off[-1] + n)
    check('8x80x69x69', torch.randn(B, K, mh, mw, generator=g) * 2, gt, label, off, 1.0)
