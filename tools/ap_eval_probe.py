"""Time the on-device mAP evaluator (yolact_amd.evaluation) against the CPU statement of the reference's (oracle/map_eval).

    python tools/ap_eval_probe.py [--out FILE.json]      # prints the JSON; --out also writes it

  * APEvaluator.add() per image at 550 x 550: R50 forward on synthetic weights (100 detections per image), 10 or 50 GT objects
    (random rectangles, masks 0/1); wall time of a run of add() calls plus the final synchronisation, per image;
  * oracle/map_eval.prep_metrics on the same postprocess output and GT on this host's CPU, per image;
  * calc_map() after 5 000 synthetic images (100 detections, 10 GT, 80 classes; records already on the device): sort + AP
    kernel + host means; and oracle/map_eval.calc_map on the same data points (exported with to_ap_data()).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rect_gt(rng, G, h, w, ncls=80):
    gt = np.zeros((G, 5))
    masks = np.zeros((G, h, w), np.uint8)
    for j in range(G):
        x0, x1 = sorted(rng.integers(0, w, 2))
        y0, y1 = sorted(rng.integers(0, h, 2))
        x1, y1 = max(x1, x0 + 8), max(y1, y0 + 8)
        gt[j] = [x0 / w, y0 / h, x1 / w, y1 / h, rng.integers(0, ncls)]
        masks[j, y0:y1, x0:x1] = 1
    return gt, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    ap.add_argument('--images', type=int, default=5000)
    args = ap.parse_args()
    import bench
    from oracle import map_eval as ME
    from yolact_amd.evaluation import APEvaluator
    from yolact_amd.layers.box_utils import mask_bits
    from yolact_amd.layers.output_utils import postprocess
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    res = {'host_cpus': os.cpu_count(), 'torch_threads': torch.get_num_threads()}
    S, B = 550, 8
    net, _ = bench.build_model(dev, S)
    x = torch.from_numpy(rng.random((B, 3, S, S), dtype=np.float32) * 2 - 1).to(dev)
    with torch.no_grad():
        preds = net(x)
    torch.cuda.synchronize()
    res['detections_per_image'] = [int(p['detection']['score'].shape[0]) if p['detection'] is not None else 0 for p in preds]
    for G in (10, 50):
        gts = [rect_gt(rng, G, S, S) for _ in range(B)]
        ev = APEvaluator(80, dev)
        for b in range(B):                                           # warm-up
            ev.add(preds, gts[b][0], gts[b][1], S, S, 0, batch_idx=b)
        torch.cuda.synchronize()
        reps = 5
        t0 = time.perf_counter()
        for _ in range(reps):
            for b in range(B):
                ev.add(preds, gts[b][0], gts[b][1], S, S, 0, batch_idx=b)
        torch.cuda.synchronize()
        res['add_ms_per_image_G%d' % G] = (time.perf_counter() - t0) * 1e3 / (reps * B)
        # the CPU statement on the same postprocess output
        posts = []
        for b in range(B):
            c, s, bx, m = postprocess(preds, S, S, batch_idx=b)
            posts.append((c.cpu(), s.cpu() if torch.is_tensor(s) else [t.cpu() for t in s], bx.cpu(), m.cpu()))
        apd = ME.new_ap_data(80)
        t0 = time.perf_counter()
        for b in range(B):
            ME.prep_metrics(apd, *posts[b], gts[b][0], gts[b][1].astype(np.float32), S, S)
        res['oracle_cpu_ms_per_image_G%d' % G] = (time.perf_counter() - t0) * 1e3 / B
        print(json.dumps({k: v for k, v in res.items() if k.endswith('G%d' % G)}), flush=True)
    # calc_map after many images: small masks (the AP stage does not see them), 100 detections, 10 GT each
    h, w, N, G = 16, 16, 100, 10
    ev = APEvaluator(80, dev)
    masks = (torch.rand(N, h, w, device=dev) < 0.5).float()
    bits = mask_bits(masks)
    boxes = torch.randint(0, 8, (N, 4), device=dev)
    boxes[:, 2:] += boxes[:, :2]
    gt, gm = rect_gt(rng, G, h, w)
    t0 = time.perf_counter()
    for i in range(args.images):
        cls = torch.randint(0, 80, (N,), device=dev)
        sc = torch.randint(0, 1000, (N,), device=dev).float() / 1000
        gt[:, 4] = rng.integers(0, 80, G)
        ev.add_detections(cls, sc, boxes, bits, gt, gm, h, w, 0)
    torch.cuda.synchronize()
    res['add_detections_ms_per_image_16x16'] = (time.perf_counter() - t0) * 1e3 / args.images
    ev.calc_map()                                                    # warm-up (sort kernels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    maps = ev.calc_map()
    res['calc_map_ms_after_%d_images' % args.images] = (time.perf_counter() - t0) * 1e3
    data = ev.to_ap_data()
    apd = ME.new_ap_data(80)
    for typ in ('box', 'mask'):
        for k in range(10):
            for c in range(80):
                apd[typ][k][c].data_points = list(data[typ][k][c].data_points)
                apd[typ][k][c].num_gt_positives = data[typ][k][c].num_gt_positives
    t0 = time.perf_counter()
    ref = ME.calc_map(apd, 80)
    res['oracle_cpu_calc_map_ms_after_%d_images' % args.images] = (time.perf_counter() - t0) * 1e3
    res['calc_map_equal_to_oracle'] = ref == ev.calc_map(rounded=False)
    res['records'] = int(ev._n)
    res['mask_map_all'] = maps['mask']['all']
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
