#!/usr/bin/env python3
"""Time the opt-in fp16x2 weight gradient (ymi_conv_wgrad_nhwc_h2, csrc/conv_wgrad_h2.hip) against the default
ymi_conv_wgrad_nhwc_f32 on the shapes one yolact_resnet50 / yolact_plus step runs at B = 8, 550 x 550, and one Trainer iteration in each
mode:

  kernels   per shape, in one process: the fp32 entry twice in a row first (the distance of the two medians is the spread a repeated
            measurement of the SAME kernel shows), then the fp32 entry and the new one alternating call by call.  HIP events around
            each call (all launches of an entry), WARMUP warm-ups, medians of REPS.  The new kernel counts as faster only if the medians
            differ by more than the spread; `dw_max_rel_difference` is max |dw_h2 - dw_f32| / max |dw_f32| on N(0,1) data.
  step      one training iteration (tools/train_step_probe.py's phases, the forward inside train_ops.wgrad_mode(mode)) with
            --mode fp32, again with fp32, then with fp16x2, each in a process of its own.

Without --step every step runs in a process of its own under its own time limit, one after the other; the first that fails or runs out
of time ends the probe, and nothing more is started on the GPU.

    python tools/wgrad_h2_probe.py [--batch 8] [--reps 20] [--warmup 5] [--step kernels|step] [--mode fp32|fp16x2]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

STEPS = (('kernels', None, 420), ('step', 'fp32', 420), ('step', 'fp32', 420), ('step', 'fp16x2', 420))   # (step, mode, seconds)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (what, H = W of x, Cin, Cout, k, stride)
SHAPES = (('3x3 256 -> 256 (heads, FPN)', 69, 256, 256, 3, 1),
          ('1x1 64 -> 256 (layer1 conv3)', 138, 64, 256, 1, 1),
          ('3x3 / s2 128 -> 128 (layer2 entry)', 138, 128, 128, 3, 2),
          ('3x3 512 -> 512 (layer4 conv2)', 18, 512, 512, 3, 1),
          ('1x1 1024 -> 2048 (layer4 shortcut)', 18, 1024, 2048, 1, 1),
          ('3x3 256 -> 351 (head bbox + conf + mask)', 69, 256, 351, 3, 1),
          ('3x3 256 -> 351 (head, P7)', 5, 256, 351, 3, 1),
          ('1x1 1152 -> 128 (DCN column GEMM, 9 x 128)', 69, 1152, 128, 1, 1))


def event_us(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def step_kernels(a, torch):
    from yolact_amd import _lib as L
    from yolact_amd.layers import _loss_common as LC
    dev, lib, s = 'cuda:0', L.lib(), L.stream_ptr()
    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    for what, S, Cin, Cout, k, stride in SHAPES:
        B, ldg = a.batch, (Cout + 31) // 32 * 32
        So = (S + 2 * (k // 2) - k) // stride + 1
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(B, S, S, Cin, generator=gen).to(dev)
        g = torch.zeros(B, So, So, ldg)
        g[..., :Cout] = torch.randn(B, So, So, Cout, generator=gen)
        g = g.to(dev)
        arms = {}
        for mode, entry, kind in (('fp32', lib.ymi_conv_wgrad_nhwc_f32, 'CONV_WGRAD'), ('fp16x2', lib.ymi_conv_wgrad_nhwc_h2, 'CONV_WGRAD_H2')):
            d = L.ConvWgradDesc()
            dw, db = torch.empty(k * k * Cin, Cout, device=dev), torch.empty(Cout, device=dev)
            d.x, d.g, d.dw, d.db = x.data_ptr(), g.data_ptr(), dw.data_ptr(), db.data_ptr()
            d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, S, S, Cin, Cout, ldg, k, k, k // 2, stride
            ws = LC.workspace(kind, d, dev)
            d.ws_bytes = ws.numel()
            arms[mode] = (lambda d=d, entry=entry, mode=mode: L.check(entry(C.byref(d), s), mode), dw, db, ws, d)
        f32, h2 = arms['fp32'][0], arms['fp16x2'][0]
        for _ in range(a.warmup):
            f32()
            h2()
        torch.cuda.synchronize()
        diff = float((arms['fp16x2'][1] - arms['fp32'][1]).abs().max() / arms['fp32'][1].abs().max())
        first = statistics.median(event_us(torch, f32) for _ in range(a.reps))
        second = statistics.median(event_us(torch, f32) for _ in range(a.reps))
        t32, t16 = [], []
        for _ in range(a.reps):
            t32.append(event_us(torch, f32))
            t16.append(event_us(torch, h2))
        m32, m16 = statistics.median(t32), statistics.median(t16)
        spread = max(abs(first - second), abs(first - m32), abs(second - m32))
        flops = 2.0 * B * So * So * k * k * Cin * Cout
        print(json.dumps({'probe': 'wgrad %s at %d x %d x %d' % (what, B, S, S), 'fp32_first_us': round(first, 1),
                          'fp32_again_us': round(second, 1), 'fp32_alternating_us': round(m32, 1), 'spread_us': round(spread, 1),
                          'fp16x2_us': round(m16, 1), 'fp16x2_min_us': round(min(t16), 1), 'fp32_min_us': round(min(t32), 1),
                          'fp32_tflops': round(flops / m32 * 1e-6, 1), 'fp16x2_tflops': round(flops / m16 * 1e-6, 1),
                          'fp32_over_fp16x2': round(m32 / m16, 2), 'fp16x2_faster_by_more_than_the_spread': bool(m32 - m16 > spread),
                          'dw_max_rel_difference': diff}), flush=True)


def step_step(a, torch):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train_step_probe as TS
    from yolact_amd.layers import train_ops
    from yolact_amd.training import Trainer
    from yolact_amd.utils.augmentations import SSDAugmentation
    a.size = 550
    net = TS.build(torch, a)
    tr = Trainer(net, wgrad=a.mode)
    aug = SSDAugmentation()
    dev = [(torch.from_numpy(i).cuda(), torch.from_numpy(m).cuda(), b, l) for i, m, b, l in TS.synth_items(np, a.batch)]
    for seed in range(1, 50):          # a draw that leaves every image at least one box (MultiBoxLoss takes no empty target)
        np.random.seed(seed)
        if all(t.shape[0] > 0 for t in aug.batch(dev)[1]):
            break
    else:
        raise RuntimeError('no seed below 50 keeps a box in every image')
    np.random.seed(seed)
    images, targets, masks, num_crowds = aug.batch(dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    names = ('forward', 'loss', 'backward', 'optimiser')
    rows = {k: [] for k in names + ('step',)}
    for i in range(a.warmup + a.reps):
        e = [ev() for _ in range(5)]
        e[0].record()
        with train_ops.wgrad_mode(a.mode):
            preds = net.forward_train(images, tr.batch_stats)
        e[1].record()
        losses = tr.criterion(net, preds, targets, masks, num_crowds)
        loss = sum(losses.values())
        e[2].record()
        loss.backward()
        e[3].record()
        tr.optimizer.step(loss)
        e[4].record()
        e[4].synchronize()
        if i >= a.warmup:
            for j, k in enumerate(names):
                rows[k].append(e[j].elapsed_time(e[j + 1]) * 1e3)
            rows['step'].append(e[0].elapsed_time(e[4]) * 1e3)
    rec = {'probe': 'one training iteration without the augmentation, yolact_resnet50_config, B %d, 550 x 550, wgrad %s' % (a.batch, a.mode),
           'total_loss': round(float(loss.detach()), 4), 'skipped': int(tr.optimizer.skipped.item())}
    for k, v in rows.items():
        rec[k + '_us'] = round(statistics.median(v), 1)
        rec[k + '_min_us'] = round(min(v), 1)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step', choices=['kernels', 'step'])
    ap.add_argument('--mode', choices=['fp32', 'fp16x2'], default='fp32')
    a = ap.parse_args()
    if a.step is None:
        for step, mode, limit in STEPS:
            cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(a.batch),
                   '--reps', str(a.reps), '--warmup', str(a.warmup)] + (['--mode', mode] if mode else [])
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(json.dumps({'probe': step, 'failed': rc}), flush=True)
                sys.exit(rc)
        return
    sys.path.insert(0, ROOT)
    import torch
    {'kernels': step_kernels, 'step': step_step}[a.step](a, torch)


if __name__ == '__main__':
    main()
