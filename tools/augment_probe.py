#!/usr/bin/env python3
"""Time SSDAugmentation.batch (yolact_amd/utils/augmentations.py, csrc/augment.hip) on a batch of synthetic COCO-sized frames: 8 images
of 640 x 480 uint8 BGR with about 7 instances each, already on the GPU with their masks, to 550 x 550.

  batch    SSDAugmentation.batch end to end (the draws on the host, the table copy, the two launches), under a fixed seed per repeat so
           that every repeat does the same work; the host part alone (draw_augmentation for the 8 items) is timed with a wall clock.
  kernels  ymi_ssd_augment_f32 alone on the same records (SSDAugmentation.apply with the parameters drawn once).
  bytes    what the two launches must move at the least: every source pixel and every kept mask inside the crop once, every output
           element once; and the same at the calibrated copy bandwidth (ymi_calib_hbm_copy) as a time.
  parity   the kernel's largest distance from the float64 restatement of tests/augment_ref.py on this batch, and the float32
           restatement's (normalised units); the masks' exact equality.

HIP events around each call, WARMUP warm-ups, the median and the least of REPS.  One JSON line per measurement.

    python tools/augment_probe.py [--batch 8] [--height 480] [--width 640] [--instances 7] [--reps 20] [--warmup 5] [--skip-parity]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn, warmup, reps):
    """-> (median, least, largest) in microseconds."""
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
    return statistics.median(ts), min(ts), max(ts)


def hbm_gbps(torch, L):
    lib, s = L.lib(), L.stream_ptr()
    n = (1 << 30) // 4
    src = torch.empty(n, dtype=torch.float32, device='cuda:0').normal_()
    dst = torch.empty_like(src)
    by = C.c_double()

    def copy():
        L.check(lib.ymi_calib_hbm_copy(src.data_ptr(), dst.data_ptr(), n, C.byref(by), s), 'ymi_calib_hbm_copy')
    med, _, _ = timed(torch, copy, 2, 10)
    return by.value / med * 1e-3


def synth_items(np, a):
    """a.batch x (image uint8 [h,w,3], masks uint8 [n,h,w], relative boxes [n,4], labels): rectangles with an ellipse inside."""
    rng = np.random.RandomState(0)
    items = []
    yy, xx = np.mgrid[:a.height, :a.width]
    for _ in range(a.batch):
        img = rng.randint(0, 256, size=(a.height, a.width, 3)).astype(np.uint8)
        boxes, masks = [], []
        for _ in range(a.instances):
            bw, bh = rng.uniform(0.1, 0.6), rng.uniform(0.1, 0.6)
            x0, y0 = rng.uniform(0, 1 - bw), rng.uniform(0, 1 - bh)
            boxes.append([x0, y0, x0 + bw, y0 + bh])
            cx, cy = (x0 + bw / 2) * a.width, (y0 + bh / 2) * a.height
            masks.append((((xx - cx) / (bw * a.width / 2)) ** 2 + ((yy - cy) / (bh * a.height / 2)) ** 2 < 1).astype(np.uint8))
        items.append((img, np.stack(masks), np.array(boxes), {'num_crowds': 0, 'labels': rng.randint(0, 80, a.instances).astype(np.float64)}))
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--instances', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--skip-parity', action='store_true')
    a = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import yolact_amd
    from yolact_amd import _lib as L
    from yolact_amd.config import active_cfg
    from yolact_amd.utils.augmentations import MEANS, STD, SSDAugmentation, draw_augmentation
    if not torch.cuda.is_available():
        raise SystemExit('augment_probe: no GPU; a time is measured on the MI355X or not at all')
    print('augment_probe on %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    yolact_amd.set_cfg('yolact_base_config')
    cfg = active_cfg()
    S = int(cfg.max_size)
    host = synth_items(np, a)
    dev = [(torch.from_numpy(i).cuda(), torch.from_numpy(m).cuda(), b, l) for i, m, b, l in host]
    aug = SSDAugmentation()

    def draw_all():
        np.random.seed(1)
        return [draw_augmentation(a.height, a.width, b, l, cfg) for _, _, b, l in dev]

    def batch():
        np.random.seed(1)
        return aug.batch(dev)
    params = [p for p, _, _ in draw_all()]
    work = [(i, m, p) for (i, m, _, _), p in zip(dev, params)]
    t0 = time.perf_counter()
    for _ in range(a.reps):
        draw_all()
    host_us = (time.perf_counter() - t0) / a.reps * 1e6
    b_med, b_min, b_max = timed(torch, batch, a.warmup, a.reps)
    k_med, k_min, k_max = timed(torch, lambda: aug.apply(work, cfg=cfg), a.warmup, a.reps)
    n_kept = sum(len(p.keep) for p in params)
    # least traffic: the source pixels and kept-mask pixels that lie inside the crop once, every output element once
    src_px = 0
    for p in params:
        x0, y0, x1, y1 = p.crop
        sx = max(0, min(x1, p.off_x + p.width) - max(x0, p.off_x))
        sy = max(0, min(y1, p.off_y + p.height) - max(y0, p.off_y))
        src_px += sx * sy * (3 + len(p.keep))
    out_bytes = a.batch * 3 * S * S * 4 + n_kept * S * S * 4
    gbps = hbm_gbps(torch, L)
    rec = {'probe': 'SSDAugmentation.batch, %d x %d x %d uint8 -> %d^2, %d instances each, %d masks kept' % (
               a.batch, a.height, a.width, S, a.instances, n_kept),
           'batch_us': round(b_med, 1), 'batch_min_us': round(b_min, 1), 'batch_max_us': round(b_max, 1),
           'host_draws_us': round(host_us, 1), 'two_launches_us': round(k_med, 1), 'two_launches_min_us': round(k_min, 1),
           'two_launches_max_us': round(k_max, 1), 'images_per_s': round(a.batch / b_med * 1e6, 1),
           'bytes_read_least': src_px, 'bytes_written': out_bytes, 'hbm_copy_GBps': round(gbps, 1),
           'those_bytes_at_copy_rate_us': round((src_px + out_bytes) / gbps * 1e-3, 1)}
    print(json.dumps(rec), flush=True)
    if not a.skip_parity:
        import augment_ref as R
        images, masks = aug.apply(work, cfg=cfg)
        worst = worst32 = 0.0
        exact = True
        for (img, m, _, _), p, got, gm in zip(host, params, images, masks):
            r64 = R.augment_image(img, p, S, MEANS, STD, 0, np.float64)
            r32 = R.augment_image(img, p, S, MEANS, STD, 0, np.float32)
            worst = max(worst, float(np.abs(got.permute(1, 2, 0).cpu().numpy() - r64).max()))
            worst32 = max(worst32, float(np.abs(r32 - r64).max()))
            exact = exact and bool(np.array_equal(gm.cpu().numpy(), R.augment_masks(m, p, S).astype(np.float32)))
        print(json.dumps({'probe': 'parity on this batch (normalised units)', 'kernel_vs_float64_restatement': worst,
                          'float32_restatement_vs_float64': worst32, 'masks_equal_the_integer_rule': exact}), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
