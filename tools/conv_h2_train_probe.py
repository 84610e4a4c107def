#!/usr/bin/env python3
"""Time train_ops.conv_mode('fp16x2'), the opt-in fp16x2 forward and data gradient of the train-mode convolutions, against the default
exact-fp32 tiles on the shapes one yolact_resnet50 / yolact_plus step runs at B = 8, 550 x 550, and one Trainer iteration per pair of modes:

  kernels   per shape, in one process, the forward and (at stride 1) the data gradient as train_ops runs them.  A call is everything
            the path launches: the fp32 path's torch-permute packing and its launch; the mode's device-side pack
            (ymi_conv_pack_h2_f32), its zeroed bound slot, ymi_amax_f32 and the launch on the tile train_ops._h2_tile picks, for EVERY shape, also those
            the class rule train_ops._h2_pays leaves on the fp32 tiles (`routed_by_the_rule`): this is what the rule is judged by.  The fp32
            path twice in a row first (the distance of the medians is the spread a repeated measurement of the SAME path shows), then
            the two paths alternating call by call.  HIP events around each call, WARMUP warm-ups, medians of REPS.  The mode counts as
            faster only if the medians differ by more than the spread.  Also per shape: the packing alone on both paths, the engine
            launch alone on both (`*_launch_us`: packs and bound prepared beforehand) and, where the rule picks the pipelined kernel,
            the launch alone on the engine's own choice as an fp16x2 tile (`alt_*`), which is what the rule is judged by.
  step      one training iteration (tools/train_step_probe.py's phases) with Trainer(net, conv=..., wgrad=...), each row in a process
            of its own: (fp32, fp32), (fp32, fp32) again, (fp16x2, fp32), (fp32, fp16x2), (fp16x2, fp16x2).  After the timed
            iterations one more runs with HIP events around every packing call: `pack_total_us` is the device pack's time per step
            under the mode and the torch-permute packing's under fp32.

Without --step every step runs in a process of its own under its own time limit, one after the other; the first that fails or runs out
of time ends the probe, and nothing more is started on the GPU.

    python tools/conv_h2_train_probe.py [--batch 8] [--reps 20] [--warmup 5] [--step kernels|step] [--conv fp32|fp16x2] [--wgrad fp32|fp16x2]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

# (step, conv mode, wgrad mode, seconds)
STEPS = (('kernels', None, None, 420), ('step', 'fp32', 'fp32', 420), ('step', 'fp32', 'fp32', 420), ('step', 'fp16x2', 'fp32', 420),
         ('step', 'fp32', 'fp16x2', 420), ('step', 'fp16x2', 'fp16x2', 420))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (what, H = W of x, Cin, output widths, k, stride): the shapes of profiles/wgrad_h2_probe_b8.txt
SHAPES = (('3x3 256 -> 256 (heads, FPN)', 69, 256, (256,), 3, 1),
          ('1x1 64 -> 256 (layer1 conv3)', 138, 64, (256,), 1, 1),
          ('3x3 / s2 128 -> 128 (layer2 entry)', 138, 128, (128,), 3, 2),
          ('3x3 512 -> 512 (layer4 conv2)', 18, 512, (512,), 3, 1),
          ('1x1 1024 -> 2048 (layer4 shortcut)', 18, 1024, (2048,), 1, 1),
          ('3x3 256 -> 351 (head bbox + conf + mask)', 69, 256, (12, 243, 96), 3, 1),
          ('3x3 256 -> 351 (head, P7)', 5, 256, (12, 243, 96), 3, 1),
          ('1x1 1152 -> 128 (DCN column GEMM, 9 x 128)', 69, 1152, (128,), 1, 1),
          # the other layer classes of the ResNet-50 backbone and the pyramid's small levels: what the static rule is judged on
          ('3x3 64 -> 64 (layer1 conv2)', 138, 64, (64,), 3, 1),
          ('1x1 256 -> 64 (layer1 conv1)', 138, 256, (64,), 1, 1),
          ('3x3 128 -> 128 (layer2 conv2)', 69, 128, (128,), 3, 1),
          ('1x1 128 -> 512 (layer2 conv3)', 69, 128, (512,), 1, 1),
          ('1x1 512 -> 128 (layer2 conv1)', 69, 512, (128,), 1, 1),
          ('3x3 256 -> 256 (layer3 conv2)', 35, 256, (256,), 3, 1),
          ('1x1 256 -> 1024 (layer3 conv3)', 35, 256, (1024,), 1, 1),
          ('1x1 1024 -> 256 (layer3 conv1)', 35, 1024, (256,), 1, 1),
          ('1x1 2048 -> 512 (layer4 conv1)', 18, 2048, (512,), 1, 1),
          ('3x3 256 -> 256 (heads, P5)', 18, 256, (256,), 3, 1),
          ('3x3 256 -> 256 (heads, P6)', 9, 256, (256,), 3, 1),
          ('3x3 256 -> 351 (head, P6)', 9, 256, (12, 243, 96), 3, 1))


def event_us(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def compare(torch, a, f32, h2):
    """-> dict: the fp32 path twice for the spread, then the two alternating."""
    for _ in range(a.warmup):
        f32()
        h2()
    torch.cuda.synchronize()
    first = statistics.median(event_us(torch, f32) for _ in range(a.reps))
    second = statistics.median(event_us(torch, f32) for _ in range(a.reps))
    t32, t16 = [], []
    for _ in range(a.reps):
        t32.append(event_us(torch, f32))
        t16.append(event_us(torch, h2))
    m32, m16 = statistics.median(t32), statistics.median(t16)
    spread = max(abs(first - second), abs(first - m32), abs(second - m32))
    return {'fp32_first_us': round(first, 1), 'fp32_again_us': round(second, 1), 'fp32_alternating_us': round(m32, 1),
            'spread_us': round(spread, 1), 'fp16x2_us': round(m16, 1), 'fp16x2_min_us': round(min(t16), 1), 'fp32_min_us': round(min(t32), 1),
            'fp32_over_fp16x2': round(m32 / m16, 2), 'fp16x2_faster_by_more_than_the_spread': bool(m32 - m16 > spread),
            'fp16x2_slower_by_more_than_the_spread': bool(m16 - m32 > spread)}


def median_us(torch, a, fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    return round(statistics.median(event_us(torch, fn) for _ in range(a.reps)), 1)


def step_kernels(a, torch):
    import ctypes as C
    from yolact_amd import _lib as L
    from yolact_amd.layers import train_ops as TO
    dev = 'cuda:0'
    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    rule = TO._h2_tile
    seen = []

    def recording_rule(d):
        seen.append(rule(d))
        return seen[-1]

    def engine_choice(d):
        tile = L.lib().ymi_conv_pick_tile(C.byref(d))
        return (L.TILE_64x32_K2 if tile == L.TILE_128x32 else tile) | L.TILE_H2
    for what, S, Cin, couts, k, stride in SHAPES:
        B, ctot, pad = a.batch, sum(couts), k // 2
        ldg = (ctot + 31) // 32 * 32
        So = (S + 2 * pad - k) // stride + 1
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(B, S, S, Cin, generator=gen).to(dev)
        ws = [(torch.randn(co, Cin, k, k, generator=gen) * (2.0 / (k * k * Cin)) ** 0.5).to(dev) for co in couts]
        bias = torch.randn(ctot, generator=gen).to(dev) if len(couts) > 1 else None
        g = torch.zeros(B, So, So, ldg)
        g[..., :ctot] = torch.randn(B, So, So, ctot, generator=gen)
        g = g.to(dev)
        ys, segs, n0 = [], [], 0
        for i, co in enumerate(couts):
            ys.append(torch.empty(B, So, So, co, device=dev))
            segs.append((n0, n0 + co, L.ACT_TANH if i == 2 else L.ACT_NONE, ys[-1]))
            n0 += co
        dx = torch.empty(B, S, S, Cin, device=dev)
        dseg = [(0, Cin, L.ACT_NONE, dx)]
        flops = 2.0 * B * So * So * k * k * Cin * ctot

        def forward(mode, packed=None):
            if mode == 'fp16x2':
                planes, winv = packed or TO._pack_h2(ws, Cin, k, 0)
                TO._engine_conv(x, Cin, planes, bias, Cin, ctot, k, pad, segs, stride=stride, h2=(planes, winv))
            else:
                TO._engine_conv(x, Cin, packed if packed is not None else TO._pack_forward(TO._cat_f32(ws)), bias, Cin, ctot, k, pad, segs,
                                stride=stride)

        def dgrad(mode, packed=None):
            if mode == 'fp16x2':
                planes, winv = packed or TO._pack_h2(ws, Cin, k, 1, ldg)
                TO._engine_conv(g, ldg, planes, None, ldg, Cin, k, k - 1 - pad, dseg, h2=(planes, winv))
            else:
                TO._engine_conv(g, ldg, packed if packed is not None else TO._pack_dgrad(TO._cat_f32(ws), ldg), None, ldg, Cin, k,
                                k - 1 - pad, dseg)
        passes = [('forward', forward, lambda: TO._pack_forward(TO._cat_f32(ws)), lambda: TO._pack_h2(ws, Cin, k, 0), ys[0])]
        if stride == 1:
            passes.append(('dx', dgrad, lambda: TO._pack_dgrad(TO._cat_f32(ws), ldg), lambda: TO._pack_h2(ws, Cin, k, 1, ldg), dx))
        for which, run, pack32, pack16, out in passes:
            TO._h2_tile = recording_rule
            del seen[:]
            run('fp32')
            ref = out.clone()
            run('fp16x2')
            diff = float((out - ref).abs().max() / ref.abs().max())
            tile = seen[-1]
            rec = {'probe': '%s %s at %d x %d x %d' % (which, what, B, S, S), 'tile': L.TILE_NAMES.get(tile, str(tile)),
                   'routed_by_the_rule': bool(TO._h2_pays(k))}
            rec.update(compare(torch, a, lambda: run('fp32'), lambda: run('fp16x2')))
            rec['fp32_tflops'] = round(flops / rec['fp32_alternating_us'] * 1e-6, 1)
            rec['fp16x2_tflops'] = round(flops / rec['fp16x2_us'] * 1e-6, 1)
            rec['max_rel_difference'] = diff
            rec['fp32_pack_us'], rec['fp16x2_pack_us'] = median_us(torch, a, pack32), median_us(torch, a, pack16)
            p32, p16 = pack32(), pack16()
            rec['fp32_launch_us'] = median_us(torch, a, lambda: run('fp32', p32))
            rec['fp16x2_launch_us'] = median_us(torch, a, lambda: run('fp16x2', p16))         # (with the bound's two launches)
            if tile & L.TILE_DCNP:
                TO._h2_tile = engine_choice
                del seen[:]
                rec['alt_fp16x2_launch_us'] = median_us(torch, a, lambda: run('fp16x2', p16))
                d = L.ConvDesc()
                d.B, d.Ho, d.Wo, d.Cout = B, (So if which == 'forward' else S), (So if which == 'forward' else S), (ctot if which == 'forward' else Cin)
                rec['alt_tile'] = L.TILE_NAMES.get(engine_choice(d), '?')
            TO._h2_tile = rule
            print(json.dumps(rec), flush=True)


def step_step(a, torch):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train_step_probe as TS
    from yolact_amd.layers import train_ops as TO
    from yolact_amd.training import Trainer
    from yolact_amd.utils.augmentations import SSDAugmentation
    a.size = 550
    net = TS.build(torch, a)
    tr = Trainer(net, wgrad=a.wgrad, conv=a.conv)
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

    def iteration():
        e = [ev() for _ in range(5)]
        e[0].record()
        with TO.wgrad_mode(a.wgrad), TO.conv_mode(a.conv):
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
        return e, loss
    for i in range(a.warmup + a.reps):
        e, loss = iteration()
        if i >= a.warmup:
            for j, k in enumerate(names):
                rows[k].append(e[j].elapsed_time(e[j + 1]) * 1e3)
            rows['step'].append(e[0].elapsed_time(e[4]) * 1e3)
    rec = {'probe': 'one training iteration without the augmentation, yolact_resnet50_config, B %d, 550 x 550, conv %s, wgrad %s'
                    % (a.batch, a.conv, a.wgrad),
           'total_loss': round(float(loss.detach()), 4), 'skipped': int(tr.optimizer.skipped.item())}
    for k, v in rows.items():
        rec[k + '_us'] = round(statistics.median(v), 1)
        rec[k + '_min_us'] = round(min(v), 1)
    # one more iteration with events around every packing call of the path
    pairs = []

    def timed(fn):
        def wrapper(*args, **kw):
            p = (ev(), ev())
            p[0].record()
            out = fn(*args, **kw)
            p[1].record()
            pairs.append(p)
            return out
        return wrapper
    packers = ('_pack_h2',) if a.conv == 'fp16x2' else ('_pack_forward', '_pack_dgrad')
    saved = {n: getattr(TO, n) for n in packers}
    for n in packers:
        setattr(TO, n, timed(saved[n]))
    try:
        iteration()
    finally:
        for n in packers:
            setattr(TO, n, saved[n])
    torch.cuda.synchronize()
    rec['pack_calls'] = len(pairs)
    rec['pack_total_us'] = round(sum(p[0].elapsed_time(p[1]) for p in pairs) * 1e3, 1)
    rec['pack_what'] = 'ymi_conv_pack_h2_f32' if a.conv == 'fp16x2' else 'torch permute (_pack_forward, _pack_dgrad)'
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step', choices=['kernels', 'step'])
    ap.add_argument('--conv', choices=['fp32', 'fp16x2'], default='fp32')
    ap.add_argument('--wgrad', choices=['fp32', 'fp16x2'], default='fp32')
    a = ap.parse_args()
    if a.step is None:
        for step, conv, wgrad, limit in STEPS:
            cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(a.batch),
                   '--reps', str(a.reps), '--warmup', str(a.warmup)] + (['--conv', conv, '--wgrad', wgrad] if conv else [])
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
