#!/usr/bin/env python3
"""Time the train-mode heads (Yolact.forward_heads, csrc/conv_train.hip):

  (b) the weight gradient of one 3x3 256 -> 256 layer at 8 x 69 x 69 by ymi_conv_wgrad_nhwc_f32 (matrix cores) and by
      ymi_conv2d_bwd_nhwc_f32 (dw and db only; the thread-per-element kernel of csrc/maskiou_loss.hip).  The new kernel counts as
      faster only if the medians differ by more than the sum of the two spreads (largest minus least of the REPS timings).
  (a) forward + backward of forward_heads at B = 8 on the 550 x 550 pyramid (69, 35, 18, 9, 5) for yolact_base and yolact_plus_base,
      against the same composition in torch ops (tests/heads_train_ref.heads_ref with autograd) on the same GPU.  Recorded, not gated.

HIP events around each call, WARMUP warm-ups, the median and the least of REPS, as tools/class_loss_probe.py does.  The priors are
host constants of both arms, made before the timed calls.  (b) runs first; one line per measurement.

    python tools/heads_train_probe.py [--batch 8] [--reps 20] [--warmup 5] [--skip-torch]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import heads_train_ref as H  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import _loss_common as LC  # noqa: E402

PYRAMID = (69, 35, 18, 9, 5)


def timed(fn, warmup, reps):
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


def wgrad_probe(a, dev):
    B, S, Cin, Cout, k = a.batch, 69, 256, 256, 3
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, S, S, Cin, generator=g).to(dev)
    dy = torch.randn(B, S, S, Cout, generator=g).to(dev)
    lib, s = L.lib(), L.stream_ptr()

    new = L.ConvWgradDesc()
    dw_new = torch.empty(k * k * Cin, Cout, device=dev)
    db_new = torch.empty(Cout, device=dev)
    new.x, new.g, new.dw, new.db = x.data_ptr(), dy.data_ptr(), dw_new.data_ptr(), db_new.data_ptr()
    new.B, new.H, new.W, new.Cin, new.Cout, new.ldg, new.kh, new.kw, new.pad = B, S, S, Cin, Cout, Cout, k, k, 1
    ws_new = LC.workspace('CONV_WGRAD', new, dev)
    new.ws_bytes = ws_new.numel()

    old = L.ConvBwdDesc()
    dw_old = torch.empty(k * k * Cin, Cout, device=dev)
    db_old = torch.empty(Cout, device=dev)
    old.x, old.dy, old.dw, old.db = x.data_ptr(), dy.data_ptr(), dw_old.data_ptr(), db_old.data_ptr()
    old.B, old.H, old.W, old.Cin, old.Ho, old.Wo, old.Cout = B, S, S, Cin, S, S, Cout
    old.kh, old.kw, old.stride, old.pad, old.relu = k, k, 1, 1, 0
    ws_old = LC.workspace('CONV_BWD', old, dev)
    old.ws_bytes = ws_old.numel()

    def run_new():
        L.check(lib.ymi_conv_wgrad_nhwc_f32(C.byref(new), s), 'ymi_conv_wgrad_nhwc_f32')

    def run_old():
        L.check(lib.ymi_conv2d_bwd_nhwc_f32(C.byref(old), s), 'ymi_conv2d_bwd_nhwc_f32')

    run_new()
    run_old()
    torch.cuda.synchronize()
    agree = float((dw_new - dw_old).abs().max() / dw_old.abs().max())
    n_med, n_min, n_max = timed(run_new, a.warmup, a.reps)
    o_med, o_min, o_max = timed(run_old, a.warmup, a.reps)
    flops = 2.0 * B * S * S * k * k * Cin * Cout
    spread = (n_max - n_min) + (o_max - o_min)
    print(json.dumps({'probe': 'wgrad 3x3 %d -> %d at %d x %d x %d' % (Cin, Cout, B, S, S),
                      'new_us': round(n_med, 1), 'new_min_us': round(n_min, 1), 'new_max_us': round(n_max, 1),
                      'old_us': round(o_med, 1), 'old_min_us': round(o_min, 1), 'old_max_us': round(o_max, 1),
                      'new_tflops': round(flops / n_med * 1e-6, 1), 'old_tflops': round(flops / o_med * 1e-6, 1),
                      'old_over_new': round(o_med / n_med, 2), 'spread_us': round(spread, 1),
                      'new_faster_by_more_than_the_spread': bool(o_med - n_med > spread), 'dw_max_rel_difference': agree}), flush=True)


def heads_probe(a, dev, config):
    yolact_amd.set_cfg(config)
    cfg = yolact_amd.config.cfg
    from yolact_amd.yolact import Yolact
    net = Yolact()
    for m in (net.proto_net, net.prediction_layers, net.semantic_seg_conv):
        m.to(dev)
    spec = H.spec_of(cfg)
    names = H.param_names(spec)
    named = dict(net.named_parameters())
    plist = [named[n] for n in names]
    g = torch.Generator().manual_seed(1)
    leaves = [torch.randn(a.batch, 256, s, s, generator=g).to(dev).requires_grad_(True) for s in PYRAMID]
    with torch.no_grad():
        shapes = {k: v.shape for k, v in net.forward_heads(leaves).items() if k in H.OUT_NAMES}
    ups = {k: torch.randn(*shp, generator=g).to(dev) for k, shp in shapes.items()}

    def clear():
        for t in leaves + plist:
            t.grad = None

    def ours():
        clear()
        pred = net.forward_heads(leaves)
        sum((pred[k] * ups[k]).sum() for k in ups).backward()

    priors = H.priors_ref([(s, s) for s in PYRAMID], spec).to(dev)      # host work, made once: forward_heads caches its own too

    def torch_ops():
        clear()
        pred = H.heads_ref(leaves, {n: p for n, p in zip(names, plist)}, spec, priors=priors)
        sum((pred[k] * ups[k]).sum() for k in ups).backward()

    def ours_fwd():
        with torch.no_grad():
            net.forward_heads(leaves)

    def torch_fwd():
        with torch.no_grad():
            H.heads_ref(leaves, {n: p for n, p in zip(names, plist)}, spec, priors=priors)

    o_med, o_min, o_max = timed(ours, a.warmup, a.reps)
    rec = {'probe': 'forward_heads forward + backward, %s, B %d, pyramid %s' % (config, a.batch, list(PYRAMID)),
           'ours_us': round(o_med, 1), 'ours_min_us': round(o_min, 1), 'ours_max_us': round(o_max, 1),
           'ours_forward_only_us': round(timed(ours_fwd, a.warmup, a.reps)[0], 1)}
    if not a.skip_torch:
        t_med, t_min, t_max = timed(torch_ops, a.warmup, a.reps)
        rec.update({'torch_ops_us': round(t_med, 1), 'torch_ops_min_us': round(t_min, 1), 'torch_ops_max_us': round(t_max, 1),
                    'torch_ops_forward_only_us': round(timed(torch_fwd, a.warmup, a.reps)[0], 1),
                    'torch_over_ours': round(t_med / o_med, 2)})
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--skip-torch', action='store_true')
    a = ap.parse_args()
    dev = 'cuda:0'
    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    wgrad_probe(a, dev)
    for config in ('yolact_base_config', 'yolact_plus_base_config'):
        heads_probe(a, dev, config)


if __name__ == '__main__':
    main()
