#!/usr/bin/env python3
"""Time the lincomb mask loss, forward + backward, at B = 8, 138 x 138, 100 instances per image: ymi_mask_loss_f32 through
yolact_amd.layers.mask_loss.mask_loss next to the same function composed from PyTorch operations on the same device (the
reference's formulation, multibox_loss.py:558-627: per image matmul, sigmoid, crop, binary_cross_entropy, the ROI normalisation).

HIP events around loss + backward, WARMUP warm-ups, the median of REPS; peak device memory above the inputs for both (the
composed form keeps several [138,138,100] tensors per image alive for its backward).  Recorded, not gated.

    python tools/mask_loss_probe.py [--batch 8] [--n 100] [--size 138] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolact_amd.layers.mask_loss import mask_loss  # noqa: E402
from dcn_bwd_probe import timed  # noqa: E402

ALPHA = 6.125


def composed(proto, coef, box, gt, gt_idx, img_off, weight):
    """The reference's code path on torch ops: one image at a time, [mh,mw,n] intermediates."""
    B, mh, mw, _ = proto.shape
    total = 0
    for b in range(B):
        j0, j1 = img_off[b], img_off[b + 1]
        if j1 == j0:
            continue
        c, bx = coef[j0:j1], box[j0:j1]
        mask_t = gt[gt_idx[j0:j1].long()].permute(1, 2, 0).float()
        pred = torch.sigmoid(proto[b] @ c.t())
        x1 = torch.clamp(torch.min(bx[:, 0] * mw, bx[:, 2] * mw) - 1, min=0)
        x2 = torch.clamp(torch.max(bx[:, 0] * mw, bx[:, 2] * mw) + 1, max=mw)
        y1 = torch.clamp(torch.min(bx[:, 1] * mh, bx[:, 3] * mh) - 1, min=0)
        y2 = torch.clamp(torch.max(bx[:, 1] * mh, bx[:, 3] * mh) + 1, max=mh)
        cols = torch.arange(mw, device=proto.device, dtype=x1.dtype).view(1, -1, 1)
        rows = torch.arange(mh, device=proto.device, dtype=x1.dtype).view(-1, 1, 1)
        keep = (cols >= x1.view(1, 1, -1)) & (cols < x2.view(1, 1, -1)) & (rows >= y1.view(1, 1, -1)) & (rows < y2.view(1, 1, -1))
        pred = pred * keep.float()
        pre = F.binary_cross_entropy(torch.clamp(pred, 0, 1), mask_t, reduction='none')
        pre = pre.sum(dim=(0, 1)) / ((bx[:, 2] - bx[:, 0]) * mw) / ((bx[:, 3] - bx[:, 1]) * mh) * (mh * mw)
        total = total + torch.sum(pre * weight[j0:j1])
    return total * ALPHA / mh / mw


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--n', type=int, default=100)
    ap.add_argument('--size', type=int, default=138)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    B, n, S = a.batch, a.n, a.size
    N, n_gt = B * n, 8
    proto = (torch.relu(torch.randn(B, S, S, 32, generator=g)) * 0.5).to(dev).requires_grad_(True)
    coef = (torch.tanh(torch.randn(N, 32, generator=g)) * 0.5).to(dev).requires_grad_(True)
    c = 0.2 + 0.6 * torch.rand(N, 2, generator=g)
    half = 0.05 + 0.2 * torch.rand(N, 2, generator=g)
    box = torch.cat([c - half, c + half], 1).clamp(0.0, 1.0).to(dev)
    gt = (torch.rand(B * n_gt, S, S, generator=g) > 0.7).to(torch.uint8).to(dev)
    gt_idx = (torch.randint(0, n_gt, (N,), generator=g) + torch.arange(B).repeat_interleave(n) * n_gt).to(torch.int32).to(dev)
    img_off_host = [b * n for b in range(B + 1)]
    img_off = torch.tensor(img_off_host, dtype=torch.int32, device=dev)
    weight = torch.ones(N, device=dev)

    def run_kernel():
        proto.grad = coef.grad = None
        mask_loss(proto, coef, box, gt, gt_idx, img_off, weight, alpha=ALPHA).backward()

    def run_composed():
        proto.grad = coef.grad = None
        composed(proto, coef, box, gt, gt_idx, img_off_host, weight).backward()

    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    run_kernel()
    lk, pk, ck = mask_loss(proto, coef, box, gt, gt_idx, img_off, weight, alpha=ALPHA).item(), proto.grad.clone(), coef.grad.clone()
    run_composed()
    lc = composed(proto, coef, box, gt, gt_idx, img_off_host, weight).item()
    rel = lambda x, y: ((x - y).abs().max() / y.abs().max()).item()
    agree = {'loss': abs(lk - lc) / abs(lc), 'd_proto': rel(pk, proto.grad), 'd_coef': rel(ck, coef.grad)}
    k_med, k_min = timed(run_kernel, a.warmup, a.reps)
    c_med, c_min = timed(run_composed, a.warmup, a.reps)
    k_mem, c_mem = peak_above_inputs(run_kernel), peak_above_inputs(run_composed)
    print(json.dumps({'shape': 'B%d %dx%d n%d' % (B, S, S, n), 'kernel_fwd_bwd_us': round(k_med, 1), 'kernel_min_us': round(k_min, 1),
                      'composed_fwd_bwd_us': round(c_med, 1), 'composed_min_us': round(c_min, 1),
                      'speedup': round(c_med / k_med, 2), 'kernel_peak_MB': round(k_mem / 1e6, 1),
                      'composed_peak_MB': round(c_mem / 1e6, 1), 'intermediate_MB_per_image': round(4.0 * S * S * n / 1e6, 1),
                      'kernel_vs_composed_rel': {k: float('%.2e' % v) for k, v in agree.items()}}))


if __name__ == '__main__':
    main()
