#!/usr/bin/env python3
"""Time the class loss 'C' (csrc/class_loss.hip) and the segmentation loss 'S' (csrc/segm_loss.hip), forward + backward, against
their oracles tests/class_loss_ref.py / tests/segm_loss_ref.py composed from torch ops on the same GPU: B = 8, P = 19248, C = 81
with about 100 positives per image, and segm 8 x 80 x 69 x 69 with 10 objects per image.

HIP events around each call, WARMUP warm-ups, the median of REPS, as tools/match_probe.py does.  `ours` is ohem_conf_loss /
segm_loss through autograd (loss, then backward to the logits); `torch_ops` is the oracle's loss with autograd's backward.  For
'S' the target is built inside the timed call by the reference's loop over the objects, with device ops; the labels are a host
list, so no index is read back from the device.  Recorded, not gated.

    python tools/class_loss_probe.py [--batch 8] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import class_loss_ref as CR  # noqa: E402
import segm_loss_ref as SR  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd.layers import class_loss as CL  # noqa: E402
from yolact_amd.layers import segm_loss as SL  # noqa: E402
from dcn_bwd_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    cfg = yolact_amd.CONFIGS['yolact_base_config'].copy()
    CL.active_cfg = lambda: cfg
    B, P, NC = a.batch, 19248, 81
    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__))

    conf_t = torch.zeros(B, P, dtype=torch.long)
    for b in range(B):
        perm = torch.randperm(P, generator=g)
        conf_t[b, perm[:100]] = torch.randint(1, NC, (100,), generator=g)
        conf_t[b, perm[100:400]] = -1
    conf = (torch.randn(B, P, NC, generator=g) * 2).to(dev).requires_grad_(True)
    conf_t = conf_t.to(dev)

    def ours_c():
        conf.grad = None
        CL.ohem_conf_loss(conf, conf_t).backward()

    def torch_c():
        conf.grad = None
        CR.ohem_ref(conf, conf_t, 3)['loss'].backward()

    same = torch.equal(CL.ohem_terms(conf.detach(), conf_t)['neg'], CR.ohem_ref(conf.detach(), conf_t, 3)['neg'])
    oc, oc_min = timed(ours_c, a.warmup, a.reps)
    tc, tc_min = timed(torch_c, a.warmup, a.reps)
    print(json.dumps({'term': 'C', 'shape': 'B%d P%d C%d, 100 positives per image' % (B, P, NC), 'ours_us': round(oc, 1),
                      'ours_min_us': round(oc_min, 1), 'torch_ops_us': round(tc, 1), 'torch_ops_min_us': round(tc_min, 1),
                      'torch_over_ours': round(tc / oc, 1), 'neg_equal_torch_ops': bool(same)}))

    K, mh, mw, n = 80, 69, 69, 10
    gt = torch.zeros(B * n, mh, mw, dtype=torch.uint8)
    for j in range(B * n):
        y0, x0 = torch.randint(0, mh - 8, (2,), generator=g).tolist()
        gt[j, y0:y0 + 8 + j % 30, x0:x0 + 8 + j % 23] = 1
    label = torch.randint(0, K, (B * n,), generator=g)
    off = [n * b for b in range(B + 1)]
    segm = (torch.randn(B, K, mh, mw, generator=g) * 2).to(dev).requires_grad_(True)
    gt_d, label_d = gt.to(dev), label.to(dev)
    gt_f, label_l = gt_d.float(), label.tolist()

    def build_target():
        """The reference's loop over the objects (:232-235) with device ops."""
        with torch.no_grad():
            t = torch.zeros_like(segm)
            for b in range(B):
                for j in range(off[b], off[b + 1]):
                    t[b, label_l[j]] = torch.max(t[b, label_l[j]], gt_f[j])
        return t

    assert torch.equal(build_target().cpu(), SR.segm_targets(gt, label, off, B, K, torch.float32))

    def ours_s():
        segm.grad = None
        SL.segm_loss(segm, gt_d, label_d, off, 1.0).backward()

    def torch_s():
        segm.grad = None
        t = build_target()
        x = segm
        (1.0 / (mh * mw) * (0.5 * (x + x.abs()) - x * t + torch.log1p(torch.exp(-x.abs()))).sum()).backward()

    os_, os_min = timed(ours_s, a.warmup, a.reps)
    ts, ts_min = timed(torch_s, a.warmup, a.reps)
    print(json.dumps({'term': 'S', 'shape': '%dx%dx%dx%d, %d objects per image' % (B, K, mh, mw, n), 'ours_us': round(os_, 1),
                      'ours_min_us': round(os_min, 1), 'torch_ops_us': round(ts, 1), 'torch_ops_min_us': round(ts_min, 1),
                      'torch_over_ours': round(ts / os_, 1)}))


if __name__ == '__main__':
    main()
