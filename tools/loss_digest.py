#!/usr/bin/env python3
"""One SHA-256 per output tensor of the MultiBoxLoss kernels on fixed inputs: two trees whose lines are equal add in the same order
(csrc/loss_common.h, csrc/lincomb_common.h).  Only public functions are called (match_targets, box_loss, ohem_terms, segm_terms,
mask_loss_terms, gather_instances and maskiou_loss.MaskIouInput), so the script runs unchanged on an older tree.  Per term the
smallest shapes of the GPU tests and one shape at which B * tiles > 256, where the strided loop of the final sum takes more than one
trip (mask loss: N > 256); for the two lincomb terms also the smallest shapes at which their shared skeleton takes another path.

    python tools/loss_digest.py > digests.txt
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import match_ref as R  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd.layers import class_loss as CL  # noqa: E402
from yolact_amd.layers import mask_loss as ML  # noqa: E402
from yolact_amd.layers import maskiou_loss as MIL  # noqa: E402
from yolact_amd.layers import match as M  # noqa: E402
from yolact_amd.layers import segm_loss as SL  # noqa: E402

DEV = 'cuda:0'


def emit(case, name, t):
    t = t.detach().cpu().contiguous()
    print('%-18s %-9s %-7s %-18s %s' % (case, name, str(t.dtype)[6:], list(t.shape), hashlib.sha256(t.numpy().tobytes()).hexdigest()))


def match_and_box(case, priors, targets, ncs, loc_data):
    priors, targets = priors.to(DEV), [t.to(DEV) for t in targets]
    out = M.match_targets(priors, targets, ncs, loc_data.to(DEV))
    for k in sorted(out):
        emit(case, k, out[k])
    x = loc_data.to(DEV).requires_grad_(True)
    loss = M.box_loss(x, out['loc_t'], out['pos'])['B']
    loss.backward()
    emit(case, 'box B', loss)
    emit(case, 'box d_loc', x.grad)
    return out['conf_t']


def class_terms(case, conf, conf_t):
    out = CL.ohem_terms(conf.to(DEV), conf_t.to(DEV))
    for k in sorted(out):
        emit(case, k, out[k])


def big_targets(g, n, n_crowd):
    size = torch.tensor([24.0, 48.0, 96.0, 192.0, 384.0])[torch.randint(0, 5, (n + n_crowd,), generator=g)] / 550
    size = size * (0.7 + 0.7 * torch.rand(n + n_crowd, generator=g))
    c = 0.05 + 0.9 * torch.rand(n + n_crowd, 2, generator=g)
    box = torch.cat([c - size[:, None] / 2, c + size[:, None] / 2], 1).clamp(0.0, 1.0)
    cls = torch.randint(0, 80, (n + n_crowd, 1), generator=g).float()
    cls[n:] = -1
    return torch.cat([box, cls], 1)


def segm_case(case, g, B, K, mh, mw, counts):
    n = sum(counts)
    gt = torch.zeros(n, mh, mw, dtype=torch.uint8)
    for j in range(n):
        y0, x0 = torch.randint(0, mh - 4, (1,), generator=g).item(), torch.randint(0, mw - 4, (1,), generator=g).item()
        gt[j, y0:y0 + 2 + j % 7, x0:x0 + 2 + j % 5] = 1
    label = torch.randint(0, K, (n,), generator=g)
    off = [sum(counts[:b]) for b in range(B + 1)]
    segm = torch.randn(B, K, mh, mw, generator=g) * 2
    loss, d = SL.segm_terms(segm.to(DEV), gt.to(DEV), label.to(DEV), off, 1.0)
    emit(case, 'S', loss)
    emit(case, 'd_segm', d)


def mask_terms(case, *args, **switches):
    for name, t in zip(('M', 'loss_inst', 'd_proto', 'd_coef'), ML.mask_loss_terms(*[a.to(DEV) for a in args], alpha=6.125, **switches)):
        emit(case, name, t)


def lincomb_inputs(g, B, mh, mw, counts, n_gt=3):
    """proto, coef, box, gt, gt_idx, img_off for counts[b] instances in image b.  Every fourth box is a corner of the map a few
    pixels wide, which only the first (or last) wave of a tile reaches: the other waves skip that instance; every fourth has its
    corners swapped; the rest are of all sizes."""
    N = sum(counts)
    proto = torch.relu(torch.randn(B, mh, mw, 32, generator=g)) * 0.5
    coef = torch.tanh(torch.randn(N, 32, generator=g)) * 0.5
    c = 0.05 + 0.9 * torch.rand(N, 2, generator=g)
    half = 0.02 + 0.4 * torch.rand(N, 2, generator=g) ** 2
    box = torch.cat([c - half, c + half], 1).clamp(0.0, 1.0)
    j = torch.arange(N)
    box[j % 4 == 0] = torch.tensor([0.0, 0.0, 0.12, 0.1])
    box[j % 8 == 4] = torch.tensor([0.9, 0.92, 1.0, 1.0])
    swap = j % 4 == 1
    box[swap] = box[swap][:, [2, 3, 0, 1]]
    gt = (torch.rand(B * n_gt, mh, mw, generator=g) > 0.7).to(torch.uint8)
    image = torch.arange(B).repeat_interleave(torch.tensor(counts))
    gt_idx = (torch.randint(0, n_gt, (N,), generator=g) + image * n_gt).to(torch.int32)
    img_off = torch.tensor([sum(counts[:b]) for b in range(B + 1)], dtype=torch.int32)
    return proto, coef, box, gt, gt_idx, img_off


def maskiou_input(case, g, inputs, want_proto=True, want_coef=True):
    proto, coef, box, gt, gt_idx, img_off = inputs
    proto, coef = proto.to(DEV).requires_grad_(want_proto), coef.to(DEV).requires_grad_(want_coef)
    x0, iou_t = MIL.MaskIouInput.apply(proto, coef, box.to(DEV), gt.to(DEV), gt_idx.to(DEV), img_off)
    x0.backward(torch.randn(x0.shape, generator=g).to(DEV))
    emit(case, 'x0', x0)
    emit(case, 'iou_t', iou_t)
    for name, t in (('d_proto', proto), ('d_coef', coef)):
        if t.grad is not None:
            emit(case, name, t.grad)


def main():
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    M.active_cfg = CL.active_cfg = ML.active_cfg = SL.active_cfg = lambda: cfg
    print('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))

    # the smallest shapes of the GPU tests
    t = R.load_golden()[1]['crowds']                                     # B = 3, P = 345
    match_and_box('match 3x345', t['priors'], t['targets'], t['num_crowds'], t['loc_data'])
    g = torch.Generator().manual_seed(101)
    conf = (torch.randn(2, 1290, 81, generator=g) * 2).clamp(-8, 8)
    conf_t = torch.zeros(2, 1290, dtype=torch.long)                      # image 1: no positive
    perm = torch.randperm(1290, generator=g)
    conf_t[0, perm[:40]] = torch.randint(1, 81, (40,), generator=g)
    conf_t[0, perm[40:100]] = -1
    class_terms('class 2x1290', conf, conf_t)
    segm_case('segm 3x13x11', torch.Generator().manual_seed(102), 3, 80, 13, 11, [7, 0, 70])
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'mask_loss.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    for c in meta['cases']:
        get = lambda k: torch.from_numpy(z['%s_%s' % (c['name'], k)])
        masks = [get('masks_%d' % b).float() for b in range(len(c['ns']))]
        torch.manual_seed(meta['torch_seed'])
        coef, box, gt, gt_idx, img_off, weight, _ = ML.gather_instances(get('pos'), get('idx_t'), get('mask_data'), masks,
                                                                        get('gt_box_t'), c['mh'], c['mw'], meta['masks_to_train'])
        mask_terms('mask ' + c['name'], get('proto'), coef, box, gt, gt_idx, img_off, weight)

    # B * tiles > 256: more than one trip of the final sum's strided loop
    g = torch.Generator().manual_seed(103)
    priors = R.make_priors((69, 35, 18, 9, 5), 550)
    B, P = 8, priors.size(0)
    targets = [big_targets(g, 12, 1) for _ in range(B)]
    conf_t = match_and_box('match 8x%d' % P, priors, targets, [1] * B, torch.randn(B, P, 4, generator=g) * 0.7)
    class_terms('class 8x%d' % P, torch.randn(B, P, 81, generator=g) * 2, conf_t)
    segm_case('segm 8x69x69', g, 8, 80, 69, 69, [10] * 8)                 # 8 * 19 tiles: one trip; 96 x 96: 8 * 36 tiles
    segm_case('segm 8x96x96', g, 8, 80, 96, 96, [10] * 8)
    n, S, n_gt = 100, 138, 8                                             # the inputs of tools/mask_loss_probe.py --batch 8
    g = torch.Generator().manual_seed(0)
    N = B * n
    proto = torch.relu(torch.randn(B, S, S, 32, generator=g)) * 0.5
    coef = torch.tanh(torch.randn(N, 32, generator=g)) * 0.5
    c = 0.2 + 0.6 * torch.rand(N, 2, generator=g)
    half = 0.05 + 0.2 * torch.rand(N, 2, generator=g)
    box = torch.cat([c - half, c + half], 1).clamp(0.0, 1.0)
    gt = (torch.rand(B * n_gt, S, S, generator=g) > 0.7).to(torch.uint8)
    gt_idx = (torch.randint(0, n_gt, (N,), generator=g) + torch.arange(B).repeat_interleave(n) * n_gt).to(torch.int32)
    img_off = torch.tensor([b * n for b in range(B + 1)], dtype=torch.int32)
    mask_terms('mask 8x138x138', proto, coef, box, gt, gt_idx, img_off, torch.ones(N))

    # the lincomb skeleton's paths (csrc/lincomb_common.h): two LDS rounds with a last group of 2 of 8 (the mask loss stages 320
    # instances at once, the mask-IoU input 128), one ragged tile, an image without instances, five tiles with the last ragged and
    # d_proto or d_coef not wanted, the switches off
    g = torch.Generator().manual_seed(104)
    mask_terms('mask 2x12x10 n330', *lincomb_inputs(g, 2, 12, 10, [330, 5]), 0.5 + torch.rand(335, generator=g))
    mask_terms('mask 3x13x11 plain', *lincomb_inputs(g, 3, 13, 11, [7, 0, 5]), 0.5 + torch.rand(12, generator=g), crop=False, roi_norm=False)
    maskiou_input('miou 2x15x15', g, lincomb_inputs(g, 2, 15, 15, [130, 3]))
    maskiou_input('miou 3x13x11', g, lincomb_inputs(g, 3, 13, 11, [7, 0, 5]))
    inputs = lincomb_inputs(g, 2, 33, 35, [9, 17])
    maskiou_input('miou 2x33x35 p', g, inputs, want_coef=False)
    maskiou_input('miou 2x33x35 c', g, inputs, want_proto=False)
    maskiou_input('miou 2x33x35 pc', g, inputs)
    # the inputs of tools/maskiou_loss_probe.py --batch 8 (those of the mask loss above)
    maskiou_input('miou 8x138x138', torch.Generator().manual_seed(1), (proto, coef, box, gt, gt_idx, img_off))


if __name__ == '__main__':
    main()
