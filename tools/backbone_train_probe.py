#!/usr/bin/env python3
"""Time the train-mode backbone (Yolact.forward_backbone, csrc/conv_dgrad.hip, csrc/bn_train.hip):

  (a) ymi_conv_dgrad_s2_nhwc_f32 against the zero-insert route of conv2d_down's data gradient (train_ops._data_grad: g spread over a
      zeroed H x W buffer, then the stride-1 data gradient on the conv engine; filters packed beforehand for both) on the ResNet stage entries at B = 8 and
      550 x 550: 3x3 128 -> 128 at 138 -> 69, 256 -> 256 at 69 -> 35, 512 -> 512 at 35 -> 18, and the 1x1 projection shortcuts
      256 -> 512, 512 -> 1024, 1024 -> 2048 at the same maps.  ROUNDS alternating rounds (route, kernel, route, kernel, ..), each the
      median of REPS; reported: the median of the rounds' medians, the least time seen, and the route's own spread (largest minus
      smallest round median).  The engine launch of the route alone (without the fill and the scatter) is reported too.
      REQUIREMENT (3x3 shapes): kernel median < route median - route spread.  The script prints whether it holds; it gates nothing.
  (b) ymi_bn_fwd_nhwc_f32 + ymi_bn_bwd_nhwc_f32 (batch statistics, no residual, ReLU off) against torch.nn.functional.batch_norm
      forward + backward at [8 * 138^2, 256] and [8 * 18^2, 2048], as GB/s of the least traffic (forward: x in, y out; backward: x and
      dy in, dx out: 5 * npos * C * 4 bytes).
  (c) forward + backward of forward_backbone for ResNet-101 at B = 8 on the 138 x 138 stem map, frozen BatchNorm and batch statistics,
      against the same composition in torch ops (tests/backbone_train_ref.chain_ref with autograd) on the same GPU.

HIP events around each call, WARMUP warm-ups, the median and the least of REPS.  One JSON line per measurement.

    python tools/backbone_train_probe.py [--batch 8] [--reps 20] [--warmup 5] [--rounds 4] [--skip-torch] [--only a|b|c]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import backbone_train_ref as R  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

# (kernel, Cin, Cout, H): the stage entries' conv2 and projection shortcuts at 550 x 550
DGRAD_SHAPES = [(3, 128, 128, 138), (3, 256, 256, 69), (3, 512, 512, 35), (1, 256, 512, 138), (1, 512, 1024, 69), (1, 1024, 2048, 35)]
BN_SHAPES = [(138, 256), (18, 2048)]


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


def dgrad_probe(a, dev, shape):
    k, Cin, Cout, size = shape
    B, So = a.batch, (size - 1) // 2 + 1
    gen = torch.Generator().manual_seed(0)
    g = torch.randn(B, So, So, Cout, generator=gen).to(dev)
    w = (torch.randn(Cout, Cin, k, k, generator=gen) * (2.0 / (Cout * k * k)) ** 0.5).to(dev)
    lib, s = L.lib(), L.stream_ptr()
    dx_new = torch.empty(B, size, size, Cin, device=dev)
    dx_old = torch.empty(B, size, size, Cin, device=dev)
    wpk = TO._pack_dgrad_s2(w, Cout)
    d = L.ConvDgradDesc()
    d.g, d.w, d.dx = g.data_ptr(), wpk.data_ptr(), dx_new.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, size, size, Cin, Cout, Cout, k, k, k // 2, 2
    wflip = TO._pack_dgrad(w, Cout)
    keep = {}

    def kernel():
        rc = lib.ymi_conv_dgrad_s2_nhwc_f32(C.byref(d), s)
        assert rc == 0, rc

    def route():
        gz = torch.zeros(B, size, size, Cout, dtype=torch.float32, device=dev)
        gz[:, ::2, ::2] = g
        keep['gz'] = gz
        TO._engine_conv(gz, Cout, wflip, None, Cout, Cin, k, k - 1 - k // 2, [(0, Cin, L.ACT_NONE, dx_old)])

    def engine_alone():
        TO._engine_conv(keep['gz'], Cout, wflip, None, Cout, Cin, k, k - 1 - k // 2, [(0, Cin, L.ACT_NONE, dx_old)])

    route()
    kernel()
    torch.cuda.synchronize()
    diff = float((dx_new - dx_old).abs().max() / dx_old.abs().max())
    r_med, k_med, r_min, k_min = [], [], [], []
    for _ in range(a.rounds):
        m, lo, _ = timed(route, a.warmup, a.reps)
        r_med.append(m)
        r_min.append(lo)
        m, lo, _ = timed(kernel, a.warmup, a.reps)
        k_med.append(m)
        k_min.append(lo)
    e_med, e_min, _ = timed(engine_alone, a.warmup, a.reps)
    route_us, kernel_us, spread = statistics.median(r_med), statistics.median(k_med), max(r_med) - min(r_med)
    flops = 2.0 * B * So * So * k * k * Cin * Cout
    rec = {'probe': 'dgrad %dx%d / stride 2, %d -> %d at %d x %d^2 -> %d^2' % (k, k, Cin, Cout, B, size, So),
           'kernel_us': round(kernel_us, 1), 'kernel_min_us': round(min(k_min), 1), 'kernel_round_medians_us': [round(t, 1) for t in k_med],
           'zero_insert_route_us': round(route_us, 1), 'route_min_us': round(min(r_min), 1),
           'route_round_medians_us': [round(t, 1) for t in r_med], 'route_spread_us': round(spread, 1),
           'route_engine_launch_alone_us': round(e_med, 1), 'route_engine_launch_alone_min_us': round(e_min, 1),
           'kernel_tflops': round(flops / kernel_us * 1e-6, 2), 'route_over_kernel': round(route_us / kernel_us, 2),
           'max_rel_difference': diff, 'kernel_below_route_by_more_than_its_spread': bool(kernel_us < route_us - spread),
           'kernel_below_engine_launch_alone': bool(kernel_us < e_med)}
    print(json.dumps(rec), flush=True)


def bn_probe(a, dev, size, Cc):
    npos = a.batch * size * size
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(npos, Cc, generator=gen).to(dev)
    dy = torch.randn(npos, Cc, generator=gen).to(dev)
    gamma, beta = (0.5 + torch.rand(Cc, generator=gen)).to(dev), torch.randn(Cc, generator=gen).to(dev)
    rm, rv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, invstd, dg, db = (torch.empty(Cc, device=dev) for _ in range(4))
    lib, s = L.lib(), L.stream_ptr()
    d = L.BnDesc()
    d.x, d.gamma, d.beta, d.running_mean, d.running_var = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr()
    d.y, d.mean, d.invstd, d.dy, d.dx, d.dgamma, d.dbeta = (t.data_ptr() for t in (y, mean, invstd, dy, dx, dg, db))
    d.npos, d.C, d.training, d.relu, d.eps, d.momentum = npos, Cc, 1, 0, 1e-5, 0.1
    nbytes = lib.ymi_workspace_bytes(L.WS_BN, C.byref(d))
    assert nbytes > 0, nbytes
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    d.ws, d.ws_bytes = ws.data_ptr(), int(nbytes)

    def fwd():
        rc = lib.ymi_bn_fwd_nhwc_f32(C.byref(d), s)
        assert rc == 0, rc

    def bwd():
        rc = lib.ymi_bn_bwd_nhwc_f32(C.byref(d), s)
        assert rc == 0, rc

    def both():
        fwd()
        bwd()
    f_med, f_min, _ = timed(fwd, a.warmup, a.reps)
    b_med, b_min, _ = timed(bwd, a.warmup, a.reps)
    t_med, t_min, _ = timed(both, a.warmup, a.reps)
    nb = 4.0 * npos * Cc
    rec = {'probe': 'batch norm forward + backward, batch statistics, [%d * %d^2, %d]' % (a.batch, size, Cc),
           'fwd_us': round(f_med, 1), 'fwd_min_us': round(f_min, 1), 'fwd_GBps': round(2 * nb / f_med * 1e-3, 1),
           'bwd_us': round(b_med, 1), 'bwd_min_us': round(b_min, 1), 'bwd_GBps': round(3 * nb / b_med * 1e-3, 1),
           'fwd_plus_bwd_us': round(t_med, 1), 'fwd_plus_bwd_min_us': round(t_min, 1), 'fwd_plus_bwd_GBps': round(5 * nb / t_med * 1e-3, 1)}
    if not a.skip_torch:
        xn = x.view(a.batch, size, size, Cc).permute(0, 3, 1, 2).requires_grad_(True)          # channels-last storage, as ours
        gn = dy.view(a.batch, size, size, Cc).permute(0, 3, 1, 2)
        gl, bl = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        trm, trv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)

        def run_torch():
            out = F.batch_norm(xn, trm, trv, gl, bl, True, 0.1, 1e-5)
            torch.autograd.grad(out, [xn, gl, bl], gn)
        q_med, q_min, _ = timed(run_torch, a.warmup, a.reps)
        rec.update({'torch_fwd_plus_bwd_us': round(q_med, 1), 'torch_min_us': round(q_min, 1),
                    'torch_GBps': round(5 * nb / q_med * 1e-3, 1), 'torch_over_ours': round(q_med / t_med, 2)})
    print(json.dumps(rec), flush=True)


def backbone_probe(a, dev, config, batch_stats):
    yolact_amd.set_cfg(config)
    from yolact_amd.yolact import Yolact
    torch.manual_seed(0)
    net = Yolact()
    net.backbone.to(dev)
    size = 138
    gen = torch.Generator().manual_seed(1)
    leaf = torch.randn(a.batch, 64, size, size, generator=gen).abs().to(dev).requires_grad_(True)
    plist = [p for p in net.backbone.layers.parameters()]
    with torch.no_grad():
        ups = [torch.randn(*o.shape, generator=gen).to(dev) for o in net.forward_backbone(leaf, False)]
    params = {n: t for n, t in net.backbone.state_dict().items() if n.startswith('layers.')}
    blocks = [('layers.%d.%d.' % (si, bi), blk.stride) for si, layer in enumerate(net.backbone.layers) for bi, blk in enumerate(layer)]
    ends, at = [], 0
    for layer in net.backbone.layers:
        at += len(layer)
        ends.append(at - 1)

    def clear():
        leaf.grad = None
        for t in plist:
            t.grad = None

    def ours():
        clear()
        sum((o * u).sum() for o, u in zip(net.forward_backbone(leaf, batch_stats), ups)).backward()

    def torch_ops():
        clear()
        outs = R.chain_ref(leaf, params, blocks, batch_stats)
        sum((outs[e] * u).sum() for e, u in zip(ends, ups)).backward()

    def ours_fwd():
        with torch.no_grad():
            net.forward_backbone(leaf, batch_stats)

    o_med, o_min, o_max = timed(ours, a.warmup, a.reps)
    rec = {'probe': 'forward_backbone forward + backward, %s, B %d, stem map %d^2, %s' % (config, a.batch, size,
                                                                                      'batch statistics' if batch_stats else 'frozen BN'),
           'ours_us': round(o_med, 1), 'ours_min_us': round(o_min, 1), 'ours_max_us': round(o_max, 1),
           'ours_forward_only_us': round(timed(ours_fwd, a.warmup, a.reps)[0], 1)}
    if not a.skip_torch:
        t_med, t_min, t_max = timed(torch_ops, a.warmup, a.reps)
        rec.update({'torch_ops_us': round(t_med, 1), 'torch_ops_min_us': round(t_min, 1), 'torch_ops_max_us': round(t_max, 1),
                    'torch_over_ours': round(t_med / o_med, 2)})
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--skip-torch', action='store_true')
    ap.add_argument('--only', default='abc')
    a = ap.parse_args()
    dev = 'cuda:0'
    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    if 'a' in a.only:
        for shape in DGRAD_SHAPES:
            dgrad_probe(a, dev, shape)
    if 'b' in a.only:
        for size, Cc in BN_SHAPES:
            bn_probe(a, dev, size, Cc)
    if 'c' in a.only:
        for batch_stats in (False, True):
            backbone_probe(a, dev, 'yolact_base_config', batch_stats)


if __name__ == '__main__':
    main()
