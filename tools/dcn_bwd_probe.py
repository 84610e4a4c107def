#!/usr/bin/env python3
"""Time ymi_dcn_v2_backward_f32 next to ymi_dcn_v2_forward_f32 on the three YOLACT++ DCN stage shapes at batch 8.

HIP events around each call, WARMUP warm-ups, the median of REPS; the backward with all five gradients, and its two kernels on
their own (data: gx + g_offset + g_mask; weight: gw + gbias).  Next to each time: the bytes the backward must move at least
(x, gy, gx once each, offmask twice) and the bandwidth that would be.  Recorded, not gated.

    python tools/dcn_bwd_probe.py [--batch 8] [--reps 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import dcn_v2  # noqa: E402

SHAPES = [(128, 69, 1), (256, 35, 1), (512, 18, 1)]        # Cin = Cout, map size, stride


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    for Cc, S, stride in SHAPES:
        B = a.batch
        x = torch.randn(B, S, S, Cc, generator=g).to(dev)
        w = (torch.randn(Cc, Cc, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5).to(dev)
        bias = torch.zeros(Cc, device=dev)
        om = torch.cat([torch.randn(B, S, S, 18, generator=g) * 2, torch.sigmoid(torch.randn(B, S, S, 9, generator=g))], 3).to(dev)
        gy = torch.randn(B, S, S, Cc, generator=g).to(dev)
        wd = w.permute(0, 2, 3, 1).contiguous()
        pk = dcn_v2._packed(w, bias, stride, 1, None, torch.device(dev))
        outs = {'gx': torch.empty_like(x), 'g_offset': torch.empty(B, S, S, 18, device=dev), 'g_mask': torch.empty(B, S, S, 9, device=dev),
                'gw': torch.empty_like(wd), 'gbias': torch.empty(Cc, device=dev)}

        def bwd(which):
            d = L.DcnBwdDesc()
            d.x, d.offmask, d.w, d.gy = x.data_ptr(), om.data_ptr(), wd.data_ptr(), gy.data_ptr()
            for f in which:
                setattr(d, f, outs[f].data_ptr())
            d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = B, S, S, Cc, Cc, S, S, Cc
            d.kh, d.kw, d.stride, d.pad, d.dilation, d.deformable_groups = 3, 3, stride, 1, 1, 1
            d.ldo, d.mask_is_prob, d.om_layout = 27, 1, 0
            return lambda: L.check(L.lib().ymi_dcn_v2_backward_f32(C.byref(d), L.stream_ptr()), 'backward')

        fwd, _ = timed(lambda: dcn_v2._dcn_launch(x, om, True, pk, S, S), a.warmup, a.reps)
        full, full_min = timed(bwd(list(outs)), a.warmup, a.reps)
        data, _ = timed(bwd(['gx', 'g_offset', 'g_mask']), a.warmup, a.reps)
        wgt, _ = timed(bwd(['gw', 'gbias']), a.warmup, a.reps)
        nbytes = 4 * (2 * x.numel() + gy.numel() + 2 * om.numel())
        print(json.dumps({'shape': 'B%d c%d %dx%d s%d' % (B, Cc, S, S, stride), 'forward_us': round(fwd, 1),
                          'backward_us': round(full, 1), 'backward_min_us': round(full_min, 1), 'data_kernel_us': round(data, 1),
                          'weight_kernel_us': round(wgt, 1), 'backward_over_forward': round(full / fwd, 2),
                          'min_bytes_MB': round(nbytes / 1e6, 1), 'GBps_at_min_bytes': round(nbytes / full / 1e3, 1),
                          'gflop_gcol_plus_gw': round(4.0 * B * S * S * 9 * Cc * Cc / 1e9, 1),
                          'tflops': round(4.0 * B * S * S * 9 * Cc * Cc / full / 1e6, 1)}))


if __name__ == '__main__':
    main()
