#!/usr/bin/env python3
"""Time one training iteration (yolact_amd.training.Trainer) on yolact_resnet50_config at B = 8, 550 x 550, phase by phase, and the
optimiser alone against torch's on the same tensors:

  optim   optim.SGD.step(loss) (one launch of csrc/sgd.hip: update + guard + zeroed gradients) against
          torch.optim.SGD(foreach=True).step() + zero_grad(set_to_none=False) on every parameter of the model with a gradient:
          launches (ours: counted by the optimiser; torch: kernels of a torch.profiler trace of one call), microseconds, and the bytes
          moved per second against the 6.29 TB/s copy rate of the part.  Ours moves 3 reads + 3 writes of 4 bytes per element
          (p, g, m in; p, m, zeroed g out).  Two timings each: the call on an idle device (the host's work of the call lies between
          the events: in a training step it hides behind the backward pass still running), and the device time alone from cold caches
          (3 GiB of fills queued ahead of the first event).
  phases  augment (SSDAugmentation.batch on 8 synthetic 480 x 640 images of 7 instances), forward (forward_train, batch statistics),
          loss (MultiBoxLoss), backward, optimiser (SGD.step(loss)): each between HIP events, in the order a step runs them.

HIP events around each call, WARMUP warm-ups, the median and the least of REPS.  One JSON line per measurement.  Without --step every
step runs in a process of its own under its own time limit, one after the other; the first step that fails or runs out of time ends
the probe, and nothing more is started on the GPU.

    python tools/train_step_probe.py [--batch 8] [--size 550] [--reps 20] [--warmup 5] [--step optim|phases]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

STEPS = (('optim', 240), ('phases', 420))      # (step, its time limit in seconds)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_COPY_TBPS = 6.29


def timed(torch, fn, warmup, reps, before=None, busy=None):
    """-> (median, least) in microseconds; `before` runs untimed ahead of every call.  `busy` is enqueued ahead of the first event: while
    the device works through it the host enqueues fn and the second event, so the events bracket device time alone."""
    ts = []
    for i in range(warmup + reps):
        if before is not None:
            before()
        if busy is not None:
            torch.cuda.synchronize()
            busy()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def build(torch, a):
    import yolact_amd
    yolact_amd.set_cfg('yolact_resnet50_config')
    yolact_amd.config.cfg.max_size = a.size
    from yolact_amd.yolact import Yolact
    torch.manual_seed(0)
    return Yolact().to('cuda:0')


def step_optim(a, torch):
    from yolact_amd.optim import SGD
    net = build(torch, a)
    params = list(net.parameters())
    n = sum(p.numel() for p in params)
    gen = torch.Generator(device='cuda:0').manual_seed(1)

    def fill():
        for p in params:
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.normal_(generator=gen)
    loss = torch.tensor(1.0, device='cuda:0')
    ours = SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4)
    fill()
    o_med, o_min = timed(torch, lambda: ours.step(loss), a.warmup, a.reps, before=fill)
    launches = ours.launches / (a.warmup + a.reps)      # (per step: one parameter group)
    theirs = torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-4, foreach=True)

    def torch_step():
        theirs.step()
        theirs.zero_grad(set_to_none=False)
    t_med, t_min = timed(torch, torch_step, a.warmup, a.reps, before=fill)
    # device time alone, from cold caches: 3 GiB of fills run ahead of the first event (about a millisecond, and they evict p, g and m)
    scratch = torch.empty(1 << 28, dtype=torch.float32, device='cuda:0')

    def busy():
        for _ in range(3):
            scratch.zero_()
    od_med, od_min = timed(torch, lambda: ours.step(loss), a.warmup, a.reps, before=fill, busy=busy)
    td_med, td_min = timed(torch, torch_step, a.warmup, a.reps, before=fill, busy=busy)
    nbytes = 6.0 * 4 * n
    print(json.dumps({'probe': 'SGD step + zeroed gradients, %d tensors, %d elements' % (len(params), n),
                      'ours_launches': launches, 'ours_call_on_idle_device_us': round(o_med, 1), 'ours_call_min_us': round(o_min, 1),
                      'torch_foreach_call_on_idle_device_us': round(t_med, 1), 'torch_foreach_call_min_us': round(t_min, 1),
                      'ours_device_us': round(od_med, 1), 'ours_device_min_us': round(od_min, 1),
                      'ours_TBps': round(nbytes / od_med * 1e-6, 3), 'ours_fraction_of_copy_rate': round(nbytes / od_med * 1e-6 / HBM_COPY_TBPS, 3),
                      'torch_foreach_device_us': round(td_med, 1), 'torch_foreach_device_min_us': round(td_min, 1),
                      'torch_over_ours_call': round(t_med / o_med, 2), 'torch_over_ours_device': round(td_med / od_med, 2),
                      'table_uploads': ours.uploads}), flush=True)
    # torch's launches: the device kernels of a profiler trace of one call (after the timings: the trace is not on their path)
    fill()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        torch_step()
        torch.cuda.synchronize()
    t_launches = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    print(json.dumps({'probe': 'torch.optim.SGD(foreach=True).step() + zero_grad()', 'torch_foreach_launches': t_launches}), flush=True)


def synth_items(np, batch, height=480, width=640, instances=7):
    """batch x (image uint8 [h,w,3], masks uint8 [n,h,w], relative boxes [n,4], labels): rectangles with an ellipse inside."""
    rng = np.random.RandomState(0)
    items = []
    yy, xx = np.mgrid[:height, :width]
    for _ in range(batch):
        img = rng.randint(0, 256, size=(height, width, 3)).astype(np.uint8)
        boxes, masks = [], []
        for _ in range(instances):
            bw, bh = rng.uniform(0.1, 0.6), rng.uniform(0.1, 0.6)
            x0, y0 = rng.uniform(0, 1 - bw), rng.uniform(0, 1 - bh)
            boxes.append([x0, y0, x0 + bw, y0 + bh])
            cx, cy = (x0 + bw / 2) * width, (y0 + bh / 2) * height
            masks.append((((xx - cx) / (bw * width / 2)) ** 2 + ((yy - cy) / (bh * height / 2)) ** 2 < 1).astype(np.uint8))
        items.append((img, np.stack(masks), np.array(boxes), {'num_crowds': 0, 'labels': rng.randint(0, 80, instances).astype(np.float64)}))
    return items


def step_phases(a, torch):
    import numpy as np
    from yolact_amd.training import Trainer
    from yolact_amd.utils.augmentations import SSDAugmentation
    net = build(torch, a)
    tr = Trainer(net)
    aug = SSDAugmentation()
    dev = [(torch.from_numpy(i).cuda(), torch.from_numpy(m).cuda(), b, l) for i, m, b, l in synth_items(np, a.batch)]
    for seed in range(1, 50):          # a draw that leaves every image at least one box (MultiBoxLoss takes no empty target)
        np.random.seed(seed)
        batch = aug.batch(dev)
        if all(t.shape[0] > 0 for t in batch[1]):
            break
    else:
        raise RuntimeError('no seed below 50 keeps a box in every image')

    def augment():
        np.random.seed(seed)
        return aug.batch(dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    rows = {k: [] for k in ('augment', 'forward', 'loss', 'backward', 'optimiser', 'step')}
    for i in range(a.warmup + a.reps):
        e = [ev() for _ in range(6)]
        e[0].record()
        images, targets, masks, num_crowds = augment()
        e[1].record()
        preds = net.forward_train(images, tr.batch_stats)
        e[2].record()
        losses = tr.criterion(net, preds, targets, masks, num_crowds)
        loss = sum(losses.values())
        e[3].record()
        loss.backward()
        e[4].record()
        tr.optimizer.step(loss)
        e[5].record()
        e[5].synchronize()
        if i >= a.warmup:
            for j, k in enumerate(('augment', 'forward', 'loss', 'backward', 'optimiser')):
                rows[k].append(e[j].elapsed_time(e[j + 1]) * 1e3)
            rows['step'].append(e[0].elapsed_time(e[5]) * 1e3)
    rec = {'probe': 'one training iteration, yolact_resnet50_config, B %d, %d x %d, batch statistics' % (a.batch, a.size, a.size),
           'total_loss': round(float(loss.detach()), 4), 'skipped': int(tr.optimizer.skipped.item()), 'table_uploads': tr.optimizer.uploads}
    for k, v in rows.items():
        rec[k + '_us'] = round(statistics.median(v), 1)
        rec[k + '_min_us'] = round(min(v), 1)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=550)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step', choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step is None:
        for step, limit in STEPS:
            cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(a.batch),
                   '--size', str(a.size), '--reps', str(a.reps), '--warmup', str(a.warmup)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(json.dumps({'probe': step, 'failed': rc}), flush=True)
                sys.exit(rc)
        return
    sys.path.insert(0, ROOT)
    import torch
    {'optim': step_optim, 'phases': step_phases}[a.step](a, torch)


if __name__ == '__main__':
    main()
