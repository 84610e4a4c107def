#!/usr/bin/env python3
"""Time the mask-IoU term 'I', forward + backward, at B = 8, 138 x 138 prototypes, 100 instances per image and the shipped
FastMaskIoUNet: yolact_amd.layers.maskiou_loss (ymi_maskiou_input_f32, the net on the direct convolution kernels,
ymi_maskiou_head_f32 and their backwards) next to the same term composed from PyTorch operations on the same device (the oracle's
formulation, tests/maskiou_loss_ref.py: matmul, sigmoid, crop, F.conv2d, F.max_pool2d, F.smooth_l1_loss, autograd).

HIP events around loss + backward (to proto, the coefficients and the twelve parameters), WARMUP warm-ups, median and minimum of
REPS; peak device memory above the inputs for both; the relative difference of the two results.  With --stages the kernel path is
also timed stage by stage (events around the pieces of one forward + backward).  Recorded, not gated.

    python tools/maskiou_loss_probe.py [--batch 8] [--n 100] [--size 138] [--reps 30] [--warmup 5] [--stages]
"""
import argparse
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from yolact_amd import CONFIGS, modules  # noqa: E402
from yolact_amd.layers import maskiou_loss as MIL  # noqa: E402
from dcn_bwd_probe import timed  # noqa: E402
from mask_loss_probe import peak_above_inputs  # noqa: E402

ALPHA = 25.0


def composed(proto, coef, box, gt, gt_idx, img_off, label_t, params):
    """The reference's code path on torch ops: per image matmul + sigmoid + crop, then the net, the gather and smooth L1."""
    B, mh, mw, _ = proto.shape
    xs, ts = [], []
    cols = torch.arange(mw, device=proto.device, dtype=proto.dtype).view(1, -1, 1)
    rows = torch.arange(mh, device=proto.device, dtype=proto.dtype).view(-1, 1, 1)
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
        keep = (cols >= x1.view(1, 1, -1)) & (cols < x2.view(1, 1, -1)) & (rows >= y1.view(1, 1, -1)) & (rows < y2.view(1, 1, -1))
        pred = pred * keep.float()
        xs.append(pred.permute(2, 0, 1).contiguous().unsqueeze(1))
        with torch.no_grad():
            pb = pred.gt(0.5).float()
            inter = (pb * mask_t).sum(dim=(0, 1))
            ts.append(inter / (pb.sum(dim=(0, 1)) + mask_t.sum(dim=(0, 1)) - inter))
    x, t = torch.cat(xs), torch.cat(ts)
    for i in range(0, len(params), 2):
        x = F.relu(F.conv2d(x, params[i], params[i + 1], stride=2 if params[i].shape[2] == 3 else 1))
    p = F.max_pool2d(x, kernel_size=x.shape[2:]).squeeze(-1).squeeze(-1)
    p = torch.gather(p, 1, label_t[:, None]).view(-1)
    return F.smooth_l1_loss(p, t, reduction='sum') * ALPHA


def layer_stages(net, x, warmup, reps):
    """Every layer's forward launch and its backward launches (dx + dw + db) alone, on buffers made once; the filter packing
    (torch ops), and the pool with its backward."""
    import ctypes as C
    from yolact_amd import _lib as L
    convs, geo = MIL.net_layers(net.maskiou_net)
    params = [t for m in convs for t in (m.weight, m.bias)]
    lib, s = L.lib(), L.stream_ptr()
    out = {}
    with torch.no_grad():
        acts, packed, pool = MIL._net_forward(MIL._nhwc(x), params, geo)
        for name, fn in (('pack_filters', lambda: [MIL._pack(w) for w in params[0::2]]),
                         ('net_forward_all', lambda: MIL._net_forward(acts[0], params, geo))):
            out[name + '_us'] = [round(v, 1) for v in timed(fn, warmup, reps)]
        for i, (kh, kw, stride, pad, relu) in enumerate(geo):
            xi, yi = acts[i], acts[i + 1]
            N, H, W, Cin = xi.shape
            Ho, Wo, Cout = yi.shape[1:]
            bias = params[2 * i + 1].detach().float().contiguous()
            ytmp = torch.empty_like(yi)

            def fwd():
                L.check(lib.ymi_conv2d_direct_nhwc_f32(xi.data_ptr(), packed[i].data_ptr(), bias.data_ptr(), ytmp.data_ptr(), N, H, W, Cin,
                                                       Ho, Wo, Cout, kh, kw, stride, pad, relu, s), 'conv')
            d = L.ConvBwdDesc()
            dy, dx, dw, db = torch.randn_like(yi), torch.empty_like(xi), torch.empty_like(packed[i]), torch.empty(Cout, device=x.device)
            d.x, d.w, d.y, d.dy, d.dx, d.dw, d.db = (t.data_ptr() for t in (xi, packed[i], yi, dy, dx, dw, db))
            d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, W, Cin, Ho, Wo, Cout
            d.kh, d.kw, d.stride, d.pad, d.relu = kh, kw, stride, pad, relu
            ws = MIL._ws('CONV_BWD', d, x.device)

            def bwd():
                L.check(lib.ymi_conv2d_bwd_nhwc_f32(C.byref(d), s), 'conv bwd')

            def bwd_dx():
                d.dw, d.db = None, None
                L.check(lib.ymi_conv2d_bwd_nhwc_f32(C.byref(d), s), 'conv bwd dx')
                d.dw, d.db = dw.data_ptr(), db.data_ptr()
            tag = 'layer%d_%dto%d' % (i + 1, Cin, Cout)
            out[tag + '_fwd_us'] = [round(v, 1) for v in timed(fwd, warmup, reps)]
            out[tag + '_bwd_us'] = [round(v, 1) for v in timed(bwd, warmup, reps)]
            out[tag + '_bwd_dx_only_us'] = [round(v, 1) for v in timed(bwd_dx, warmup, reps)]
            del ws
        N, H, W, Cc = acts[-1].shape
        dy, dpool = torch.empty_like(acts[-1]), torch.randn_like(pool)
        out['pool_fwd_us'] = [round(v, 1) for v in timed(lambda: L.check(lib.ymi_global_maxpool_nhwc_f32(
            acts[-1].data_ptr(), pool.data_ptr(), N, H * W, Cc, s), 'pool'), warmup, reps)]
        out['pool_bwd_us'] = [round(v, 1) for v in timed(lambda: L.check(lib.ymi_global_maxpool_bwd_nhwc_f32(
            acts[-1].data_ptr(), dpool.data_ptr(), dy.data_ptr(), N, H * W, Cc, s), 'pool bwd'), warmup, reps)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--n', type=int, default=100)
    ap.add_argument('--size', type=int, default=138)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--stages', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    B, n, S = a.batch, a.n, a.size
    N, n_gt = B * n, 8
    cfg = CONFIGS['yolact_plus_base_config'].copy()
    MIL.active_cfg = lambda: cfg
    net = modules.FastMaskIoUNet(cfg.maskiou_net, 81).to(dev)
    holder = types.SimpleNamespace(maskiou_net=net)       # mask_iou_loss takes anything with a .maskiou_net FastMaskIoUNet
    params = [t for m in net.maskiou_net if isinstance(m, torch.nn.Conv2d) for t in (m.weight, m.bias)]
    proto = (torch.relu(torch.randn(B, S, S, 32, generator=g)) * 0.5).to(dev).requires_grad_(True)
    coef = (torch.tanh(torch.randn(N, 32, generator=g)) * 0.5).to(dev).requires_grad_(True)
    c = 0.2 + 0.6 * torch.rand(N, 2, generator=g)
    half = 0.05 + 0.2 * torch.rand(N, 2, generator=g)
    box = torch.cat([c - half, c + half], 1).clamp(0.0, 1.0).to(dev)
    gt = (torch.rand(B * n_gt, S, S, generator=g) > 0.7).to(torch.uint8).to(dev)
    gt_idx = (torch.randint(0, n_gt, (N,), generator=g) + torch.arange(B).repeat_interleave(n) * n_gt).to(torch.int32).to(dev)
    label_t = torch.randint(0, 80, (N,), generator=g).to(dev)
    img_off = [b * n for b in range(B + 1)]
    leaves = [proto, coef] + params

    def clear():
        for t in leaves:
            t.grad = None

    def kernel_loss():
        x0, iou_t = MIL.MaskIouInput.apply(proto, coef, box, gt, gt_idx, img_off)
        return MIL.mask_iou_loss(holder, [x0.unsqueeze(1), iou_t, label_t])

    def run_kernel():
        clear()
        kernel_loss().backward()

    def run_composed():
        clear()
        composed(proto, coef, box, gt, gt_idx, img_off, label_t, params).backward()

    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    run_kernel()
    lk, gk = kernel_loss().item(), [t.grad.clone() for t in leaves]
    run_composed()
    lc, gc = composed(proto, coef, box, gt, gt_idx, img_off, label_t, params).item(), [t.grad.clone() for t in leaves]
    rel = lambda x, y: ((x - y).abs().max() / y.abs().max()).item()
    agree = {'loss': abs(lk - lc) / abs(lc), 'd_proto': rel(gk[0], gc[0]), 'd_coef': rel(gk[1], gc[1]),
             'd_params_max': max(rel(x, y) for x, y in zip(gk[2:], gc[2:]))}
    k_med, k_min = timed(run_kernel, a.warmup, a.reps)
    c_med, c_min = timed(run_composed, a.warmup, a.reps)
    k_mem, c_mem = peak_above_inputs(run_kernel), peak_above_inputs(run_composed)
    print(json.dumps({'shape': 'B%d %dx%d n%d' % (B, S, S, n), 'kernel_fwd_bwd_us': round(k_med, 1), 'kernel_min_us': round(k_min, 1),
                      'composed_fwd_bwd_us': round(c_med, 1), 'composed_min_us': round(c_min, 1),
                      'speedup': round(c_med / k_med, 2), 'kernel_peak_MB': round(k_mem / 1e6, 1),
                      'composed_peak_MB': round(c_mem / 1e6, 1),
                      'kernel_vs_composed_rel': {k: float('%.2e' % v) for k, v in agree.items()}}))
    if a.stages:
        with torch.no_grad():
            x0, iou_t = MIL.MaskIouInput.apply(proto, coef, box, gt, gt_idx, img_off)
        xin = x0.unsqueeze(1).detach().requires_grad_(True)
        stages = {
            'input_fwd': lambda: MIL.MaskIouInput.apply(proto.detach(), coef.detach(), box, gt, gt_idx, img_off),
            'input_fwd_bwd': lambda: MIL.MaskIouInput.apply(proto, coef, box, gt, gt_idx, img_off)[0].backward(x0),
            # (LossFunction computes the gradients its inputs want inside its forward: the parameters', and with xin also the input's)
            'net_head_fwd_bwd_params': lambda: MIL.mask_iou_loss(holder, [xin.detach(), iou_t, label_t]),
            'net_head_fwd_bwd_params_input': lambda: (clear(), MIL.mask_iou_loss(holder, [xin, iou_t, label_t]).backward()),
        }
        out = {}
        for name, fn in stages.items():
            with torch.set_grad_enabled(name != 'input_fwd'):
                med, lo = timed(fn, a.warmup, a.reps)
            out[name + '_us'] = [round(med, 1), round(lo, 1)]
        print(json.dumps({'stages_median_min': out}))
        print(json.dumps({'launches_median_min': layer_stages(net, xin.detach(), a.warmup, a.reps)}))


if __name__ == '__main__':
    main()
