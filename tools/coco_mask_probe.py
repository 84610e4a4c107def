#!/usr/bin/env python3
"""Time the two routes by which an image's ground-truth masks reach the GPU, on synthetic COCO-like items: N annotations of 10 - 80
vertices at 640 x 480, plus one RLE crowd (a compressed counts string).

  A  the host route: ann_to_mask per annotation (csrc/coco_host.cpp), np.vstack, reshape, one [n,h,w] upload -- what
     COCODetection.pull_item does by default, followed by SSDAugmentation's upload (_device_masks).
  B  ann_to_masks_device: one packed upload of vertices and counts, one ymi_coco_masks_u8 launch (csrc/coco_mask.hip).

Per route and item: the host wall time of the whole call, ending in a device synchronise (what a data loader thread pays), and the time
between two HIP events around it (what the stream sees); for B also the launch alone on a packed table.  WARMUP warm-ups, the median
and the least of REPS; A and B alternate inside one repeat.  The masks of both routes are compared byte for byte first.  One JSON line
per item.

    python tools/coco_mask_probe.py [--annotations 1 7 30] [--height 480] [--width 640] [--reps 30] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synth_item(np, rng, n, h, w, ann_to_mask, coco_rle):
    """n polygon annotations (star-shaped, 10 - 80 vertices, two-decimal coordinates; every fourth has two parts) and one crowd."""
    def blob(k, scale):
        cx, cy = rng.uniform(0.15, 0.85) * w, rng.uniform(0.15, 0.85) * h
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(0.3, 1.0, k) * scale * min(h, w)
        return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).round(2).reshape(-1).tolist()
    anns = []
    for i in range(n):
        polys = [blob(int(rng.integers(10, 81)), rng.uniform(0.08, 0.35))]
        if i % 4 == 3:
            polys.append(blob(int(rng.integers(10, 30)), 0.06))
        anns.append({'segmentation': polys})
    crowd = ann_to_mask({'segmentation': [blob(40, 0.3), blob(25, 0.2), blob(12, 0.1)]}, h, w)
    anns.append({'segmentation': {'size': [h, w], 'counts': coco_rle.rle_to_string(coco_rle.rle_encode_counts(crowd))}})
    return anns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--annotations', type=int, nargs='+', default=[1, 7, 30])
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from oracle import coco_rle
    from yolact_amd import _lib as L
    from yolact_amd.data import ann_to_mask, ann_to_masks_device
    from yolact_amd.data import coco as DC
    if not torch.cuda.is_available():
        raise SystemExit('coco_mask_probe: no GPU; a time is measured on the MI355X or not at all')
    print('coco_mask_probe on %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    dev = torch.device('cuda', 0)
    h, w = a.height, a.width
    lib = L.lib()

    def both_clocks(fn):
        """-> (host wall us including the synchronise, HIP event us)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        t1 = time.perf_counter()
        del out
        return (t1 - t0) * 1e6, e0.elapsed_time(e1) * 1e3

    for n in a.annotations:
        rng = np.random.default_rng(n)
        anns = synth_item(np, rng, n, h, w, ann_to_mask, coco_rle)

        def route_a():
            masks = np.vstack([ann_to_mask(x, h, w).reshape(-1) for x in anns]).reshape(-1, h, w)
            return torch.from_numpy(masks).to(dev)

        def route_b():
            return ann_to_masks_device(anns, h, w, dev)

        # the launch alone: the table packed once, the output and the workspace allocated once
        pk = DC.pack_annotations(anns, [(h, w)] * len(anns))
        out = torch.empty(len(anns), h, w, dtype=torch.uint8, device=dev)
        recs = (L.CocoMaskRec * len(anns))()
        for i in range(len(anns)):
            r = recs[i]
            r.out = out.data_ptr() + i * h * w
            r.kind, r.h, r.w, r.n, r.first, r.xy_first = (int(v[i]) for v in (pk.kind, pk.h, pk.w, pk.n, pk.first, pk.xy_first))
        d = L.CocoMaskDesc()
        d.recs, d.xy, d.poly_len, d.counts = recs, pk.xy.ctypes.data, pk.poly_len.ctypes.data, pk.counts.ctypes.data
        d.n, d.n_vert, d.n_poly, d.n_counts = len(anns), pk.xy.shape[0], pk.poly_len.size, pk.counts.size
        d.ws_bytes = lib.ymi_workspace_bytes(L.WS_COCO_MASK, C.byref(d))
        ws = torch.empty(int(d.ws_bytes), dtype=torch.uint8, device=dev)
        d.ws = ws.data_ptr()

        def entry():
            L.check(lib.ymi_coco_masks_u8(C.byref(d), L.stream_ptr()), 'ymi_coco_masks_u8')

        equal = bool(torch.equal(route_a(), route_b()))
        entry()
        equal = equal and bool(torch.equal(out, route_a()))
        for _ in range(a.warmup):
            route_a(), route_b(), entry()
        ta, tb, te = [], [], []
        for _ in range(a.reps):                      # alternating, so that a drift of the machine hits both routes
            ta.append(both_clocks(route_a))
            tb.append(both_clocks(route_b))
            te.append(both_clocks(entry))
        t0 = time.perf_counter()
        for _ in range(a.reps):
            DC.pack_annotations(anns, [(h, w)] * len(anns))
        pack_us = (time.perf_counter() - t0) / a.reps * 1e6
        med = lambda ts, k: round(statistics.median(t[k] for t in ts), 1)
        low = lambda ts, k: round(min(t[k] for t in ts), 1)
        rec = {'probe': '%d polygon annotations + 1 RLE crowd at %d x %d' % (n, w, h), 'masks_equal': equal,
               'vertices': int(pk.xy.shape[0]), 'counts': int(pk.counts.size),
               'upload_bytes_A': len(anns) * h * w, 'upload_bytes_B': int(d.ws_bytes),
               'A_host_route_wall_us': med(ta, 0), 'A_wall_min_us': low(ta, 0), 'A_events_us': med(ta, 1),
               'B_device_route_wall_us': med(tb, 0), 'B_wall_min_us': low(tb, 0), 'B_events_us': med(tb, 1),
               'B_pack_on_host_us': round(pack_us, 1),
               'B_entry_alone_wall_us': med(te, 0), 'B_entry_alone_events_us': med(te, 1), 'B_entry_alone_events_min_us': low(te, 1),
               'A_over_B_wall': round(statistics.median(t[0] for t in ta) / statistics.median(t[0] for t in tb), 2)}
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
