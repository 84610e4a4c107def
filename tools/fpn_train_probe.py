#!/usr/bin/env python3
"""Time the train-mode FPN (Yolact.forward_fpn, csrc/conv_train.hip):

  (a) the STRIDE-1 weight gradient of tools/heads_train_probe.py's layer (3x3 256 -> 256 at 8 x 69 x 69) alone.  With --lib PATH the
      library at PATH is timed instead of the tree's and nothing else runs: the A / B measurement between two builds (the stride became
      a template parameter of the kernel; the stride-1 instantiation must not get slower).  Alternate the two builds, one process per
      run, and compare the medians of the runs' medians against the spread of the earlier build's.
  (b) the STRIDE-2 weight gradient alone: the FPN's two downsample layers (3x3 256 -> 256 at 8 x 18 x 18 and 8 x 9 x 9), against
      torch's own weight gradient of the same convolution.
  (c) forward + backward of forward_fpn at B = 8 on the 550 x 550 shapes (512 / 1024 / 2048 channels at 69 / 35 / 18 squared, 256
      features), against the same composition in torch ops (tests/fpn_train_ref.fpn_ref with autograd) on the same GPU.

HIP events around each call, WARMUP warm-ups, the median and the least of REPS.  Recorded, nothing is gated; one line per measurement.

    python tools/fpn_train_probe.py [--batch 8] [--reps 20] [--warmup 5] [--skip-torch] [--lib PATH]
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
import fpn_train_ref as R  # noqa: E402
import yolact_amd  # noqa: E402
from yolact_amd import _lib as L  # noqa: E402

SIZES, IN_CHANNELS, NF = (69, 35, 18), (512, 1024, 2048), 256


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


def load(path):
    """The two entries the weight-gradient probes need, from the tree's library or from another build of it."""
    if path is None:
        return L.lib()
    lib = C.CDLL(path)
    lib.ymi_conv_wgrad_nhwc_f32.restype, lib.ymi_conv_wgrad_nhwc_f32.argtypes = C.c_int, [C.POINTER(L.ConvWgradDesc), C.c_void_p]
    lib.ymi_workspace_bytes.restype, lib.ymi_workspace_bytes.argtypes = C.c_int64, [C.c_int, C.c_void_p]
    return lib


def wgrad_probe(a, dev, lib, size, stride, what):
    B, Cin, Cout, k = a.batch, 256, 256, 3
    So = (size - 1) // 2 + 1 if stride == 2 else size
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, size, size, Cin, generator=g).to(dev)
    dy = torch.randn(B, So, So, Cout, generator=g).to(dev)
    d = L.ConvWgradDesc()
    dw = torch.empty(k * k * Cin, Cout, device=dev)
    db = torch.empty(Cout, device=dev)
    d.x, d.g, d.dw, d.db = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad = B, size, size, Cin, Cout, Cout, k, k, 1
    if stride == 2:
        d.stride = 2                                         # (stride 1: the field stays 0, as every caller before it had a name leaves it)
    nbytes = lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(d))
    assert nbytes > 0, nbytes
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    d.ws, d.ws_bytes = ws.data_ptr(), int(nbytes)
    s = L.stream_ptr()

    def run():
        rc = lib.ymi_conv_wgrad_nhwc_f32(C.byref(d), s)
        assert rc == 0, rc
    med, lo, hi = timed(run, a.warmup, a.reps)
    rec = {'probe': 'wgrad 3x3 / stride %d, %d -> %d at %d x %d x %d%s' % (stride, Cin, Cout, B, size, size, what),
           'us': round(med, 1), 'min_us': round(lo, 1), 'max_us': round(hi, 1),
           'tflops': round(2.0 * B * So * So * k * k * Cin * Cout / med * 1e-6, 2)}
    if stride == 2 and not a.skip_torch:
        xn, gn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
        w = torch.zeros(Cout, Cin, k, k, device=dev, requires_grad=True)
        run()
        torch.cuda.synchronize()
        ref = torch.autograd.grad(F.conv2d(xn, w, stride=2, padding=1), [w], gn)[0]
        rec['dw_max_rel_difference'] = float((dw.reshape(k, k, Cin, Cout).permute(3, 2, 0, 1) - ref).abs().max() / ref.abs().max())

        def run_torch():
            torch.autograd.grad(F.conv2d(xn, w, stride=2, padding=1), [w], gn)
        t_med, t_lo, t_hi = timed(run_torch, a.warmup, a.reps)
        rec.update({'torch_forward_plus_wgrad_us': round(t_med, 1), 'torch_min_us': round(t_lo, 1), 'torch_max_us': round(t_hi, 1)})
    print(json.dumps(rec), flush=True)


def fpn_probe(a, dev, config):
    yolact_amd.set_cfg(config)
    from yolact_amd.yolact import Yolact
    net = Yolact()
    net.fpn.to(dev)
    names = R.param_names(len(SIZES), len(net.fpn.downsample_layers))
    named = dict(net.named_parameters())
    plist = [named[n] for n in names]
    g = torch.Generator().manual_seed(1)
    leaves = [torch.randn(a.batch, c, s, s, generator=g).to(dev).requires_grad_(True) for c, s in zip(IN_CHANNELS, SIZES)]
    with torch.no_grad():
        ups = [torch.randn(*o.shape, generator=g).to(dev) for o in net.forward_fpn(leaves)]
    params = dict(zip(names, plist))

    def clear():
        for t in leaves + plist:
            t.grad = None

    def ours():
        clear()
        sum((o * u).sum() for o, u in zip(net.forward_fpn(leaves), ups)).backward()

    def torch_ops():
        clear()
        sum((o * u).sum() for o, u in zip(R.fpn_ref(leaves, params, len(net.fpn.downsample_layers)), ups)).backward()

    def ours_fwd():
        with torch.no_grad():
            net.forward_fpn(leaves)

    def torch_fwd():
        with torch.no_grad():
            R.fpn_ref(leaves, params, len(net.fpn.downsample_layers))

    o_med, o_min, o_max = timed(ours, a.warmup, a.reps)
    rec = {'probe': 'forward_fpn forward + backward, %s, B %d, %s channels at %s squared -> %d' % (config, a.batch, list(IN_CHANNELS),
                                                                                                list(SIZES), NF),
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
    ap.add_argument('--lib', default=None, help='another build of libyolact_amd.so: time the stride-1 weight gradient with it and stop')
    a = ap.parse_args()
    dev = 'cuda:0'
    print('device: %s  torch %s' % (torch.cuda.get_device_name(0), torch.__version__), flush=True)
    lib = load(a.lib)
    wgrad_probe(a, dev, lib, 69, 1, '' if a.lib is None else ' [%s]' % a.lib)
    if a.lib is not None:
        return
    for size in (18, 9):
        wgrad_probe(a, dev, lib, size, 2, '')
    fpn_probe(a, dev, 'yolact_base_config')


if __name__ == '__main__':
    main()
