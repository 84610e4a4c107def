#!/usr/bin/env python3
"""Time the train-mode stem (Yolact.forward_stem, csrc/stem_train.hip) at B = 8 on 550 x 550 images, each against the PyTorch composition
on the same GPU in the same run:

  calib   ymi_calib_hbm_copy over 1 GiB, as bench.py's box calibration times it: the memory bandwidth every byte count below is turned
          into a time with.
  wgrad   ymi_stem_wgrad_nhwc_f32 (x [8,550,550,4], g [8,275,275,64]) against torch.nn.grad.conv2d_weight on the NCHW image, and the
          time of ONE pass over its g and x bytes at the calibrated bandwidth.
  pool    ymi_maxpool_fwd_nhwc_f32 + ymi_maxpool_bwd_nhwc_f32 on [8,275,275,64] against F.max_pool2d forward + backward on the same
          channels-last storage.
  stem    forward + backward of forward_stem, frozen BatchNorm and batch statistics, against conv2d -> batch_norm -> relu -> max_pool2d
          in torch ops with autograd; forward alone too.

HIP events around each call, WARMUP warm-ups, the median and the least of REPS.  One JSON line per measurement.  Without --step every
step runs in a process of its own under its own time limit (`timeout`), one after the other; the first step that fails or runs out of
time ends the probe, and nothing more is started on the GPU.

    python tools/stem_train_probe.py [--batch 8] [--size 550] [--reps 20] [--warmup 5] [--skip-torch] [--step calib|wgrad|pool|stem]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

STEPS = (('calib', 120), ('wgrad', 180), ('pool', 120), ('stem', 240))      # (step, its time limit in seconds)
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
    med, lo, _ = timed(torch, copy, 2, 10)
    return by.value / med * 1e-3, by.value / lo * 1e-3


def step_calib(a, torch, L, TO):
    med, best = hbm_gbps(torch, L)
    print(json.dumps({'probe': 'ymi_calib_hbm_copy, 1 GiB read + 1 GiB written', 'GBps': round(med, 1), 'best_GBps': round(best, 1)}), flush=True)


def step_wgrad(a, torch, L, TO):
    import torch.nn.functional as F
    dev, B, S, Cout = 'cuda:0', a.batch, a.size, 64
    So = (S - 1) // 2 + 1
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, S, S, generator=gen).to(dev)
    x4 = F.pad(x.permute(0, 2, 3, 1), (0, 1)).contiguous()
    g = torch.randn(B, So, So, Cout, generator=gen).to(dev)
    dw = torch.empty(147, Cout, device=dev)
    lib, s = L.lib(), L.stream_ptr()
    d = L.StemWgradDesc()
    d.x, d.g, d.dw = x4.data_ptr(), g.data_ptr(), dw.data_ptr()
    d.B, d.H, d.W, d.Cout, d.ldg = B, S, S, Cout, Cout
    nbytes = lib.ymi_workspace_bytes(L.WS_STEM_WGRAD, C.byref(d))
    assert nbytes > 0, nbytes
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    d.ws, d.ws_bytes = ws.data_ptr(), int(nbytes)

    def kernel():
        rc = lib.ymi_stem_wgrad_nhwc_f32(C.byref(d), s)
        assert rc == 0, rc
    k_med, k_min, _ = timed(torch, kernel, a.warmup, a.reps)
    gbps, _ = hbm_gbps(torch, L)
    nb = 4.0 * (g.numel() + x4.numel())
    flops = 2.0 * B * So * So * 147 * Cout
    rec = {'probe': 'stem wgrad 7x7 / stride 2, 3 -> %d at %d x %d^2 -> %d^2' % (Cout, B, S, So), 'kernel_us': round(k_med, 1),
           'kernel_min_us': round(k_min, 1), 'kernel_tflops_useful': round(flops / k_med * 1e-6, 2), 'workspace_MB': round(nbytes / 2 ** 20, 1),
           'g_plus_x_MB': round(nb / 2 ** 20, 1), 'hbm_copy_GBps': round(gbps, 1), 'one_pass_over_g_and_x_us': round(nb / gbps * 1e-3, 1),
           'kernel_over_one_pass': round(k_med / (nb / gbps * 1e-3), 2)}
    if not a.skip_torch:
        gn = g.permute(0, 3, 1, 2)
        ref = torch.nn.grad.conv2d_weight(x, (Cout, 3, 7, 7), gn, stride=2, padding=3)
        kernel()
        torch.cuda.synchronize()
        rec['max_rel_difference'] = float((TO._unpack_dw(dw, 7, 3) - ref).abs().max() / ref.abs().max())
        t_med, t_min, _ = timed(torch, lambda: torch.nn.grad.conv2d_weight(x, (Cout, 3, 7, 7), gn, stride=2, padding=3), a.warmup, a.reps)
        rec.update({'torch_conv2d_weight_us': round(t_med, 1), 'torch_min_us': round(t_min, 1), 'torch_over_ours': round(t_med / k_med, 2)})
    print(json.dumps(rec), flush=True)


def step_pool(a, torch, L, TO):
    import torch.nn.functional as F
    dev, B, Cc = 'cuda:0', a.batch, 64
    S = (a.size - 1) // 2 + 1
    Sp = (S - 1) // 2 + 1
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, S, S, Cc, generator=gen).clamp_min(0).to(dev)          # behind a ReLU: half of it zeros
    dy = torch.randn(B, Sp, Sp, Cc, generator=gen).to(dev)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    lib, s = L.lib(), L.stream_ptr()

    def fwd():
        rc = lib.ymi_maxpool_fwd_nhwc_f32(x.data_ptr(), y.data_ptr(), B, S, S, Cc, s)
        assert rc == 0, rc

    def bwd():
        rc = lib.ymi_maxpool_bwd_nhwc_f32(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, S, S, Cc, s)
        assert rc == 0, rc
    f_med, f_min, _ = timed(torch, fwd, a.warmup, a.reps)
    b_med, b_min, _ = timed(torch, bwd, a.warmup, a.reps)
    gbps, _ = hbm_gbps(torch, L)
    nx, ny = 4.0 * x.numel(), 4.0 * y.numel()
    rec = {'probe': 'max-pool 3x3 / 2 / 1 forward and backward, [%d,%d,%d,%d]' % (B, S, S, Cc), 'fwd_us': round(f_med, 1),
           'fwd_min_us': round(f_min, 1), 'fwd_GBps': round((nx + ny) / f_med * 1e-3, 1), 'bwd_us': round(b_med, 1), 'bwd_min_us': round(b_min, 1),
           'bwd_GBps': round((2 * nx + ny) / b_med * 1e-3, 1), 'hbm_copy_GBps': round(gbps, 1)}
    if not a.skip_torch:
        xn = x.permute(0, 3, 1, 2).requires_grad_(True)                        # channels-last storage, as ours
        gn = dy.permute(0, 3, 1, 2)
        out = F.max_pool2d(xn, 3, 2, 1)
        (ref,) = torch.autograd.grad(out, [xn], gn, retain_graph=True)
        fwd()
        bwd()
        torch.cuda.synchronize()
        rec['forward_equal'] = bool(torch.equal(out.detach().permute(0, 2, 3, 1), y))
        rec['backward_max_abs_difference'] = float((ref.permute(0, 2, 3, 1) - dx).abs().max())
        tf_med, _, _ = timed(torch, lambda: F.max_pool2d(xn.detach(), 3, 2, 1), a.warmup, a.reps)
        tb_med, _, _ = timed(torch, lambda: torch.autograd.grad(out, [xn], gn, retain_graph=True), a.warmup, a.reps)
        rec.update({'torch_fwd_us': round(tf_med, 1), 'torch_bwd_us': round(tb_med, 1),
                    'torch_over_ours': round((tf_med + tb_med) / (f_med + b_med), 2)})
    print(json.dumps(rec), flush=True)


def step_stem(a, torch, L, TO):
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import yolact_amd
    yolact_amd.set_cfg('yolact_base_config')
    from yolact_amd.yolact import Yolact
    dev = 'cuda:0'
    torch.manual_seed(0)
    net = Yolact()
    bb = net.backbone
    bb.to(dev)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, 3, a.size, a.size, generator=gen).to(dev)
    plist = [bb.conv1.weight, bb.bn1.weight, bb.bn1.bias]
    with torch.no_grad():
        up = torch.randn(*net.forward_stem(x, False).shape, generator=gen).to(dev)
    for batch_stats in (False, True):
        def clear():
            for t in plist:
                t.grad = None

        def ours():
            clear()
            (net.forward_stem(x, batch_stats) * up).sum().backward()

        def ours_fwd():
            with torch.no_grad():
                net.forward_stem(x, batch_stats)

        def torch_ops():
            clear()
            z = F.batch_norm(F.conv2d(x, bb.conv1.weight, None, 2, 3), bb.bn1.running_mean, bb.bn1.running_var, bb.bn1.weight, bb.bn1.bias,
                             batch_stats, 0.1, 1e-5)
            (F.max_pool2d(F.relu(z), 3, 2, 1) * up).sum().backward()
        o_med, o_min, o_max = timed(torch, ours, a.warmup, a.reps)
        rec = {'probe': 'forward_stem forward + backward, B %d, %d x %d, %s' % (a.batch, a.size, a.size,
                                                                                'batch statistics' if batch_stats else 'frozen BN'),
               'ours_us': round(o_med, 1), 'ours_min_us': round(o_min, 1), 'ours_max_us': round(o_max, 1),
               'ours_forward_only_us': round(timed(torch, ours_fwd, a.warmup, a.reps)[0], 1)}
        if not a.skip_torch:
            t_med, t_min, t_max = timed(torch, torch_ops, a.warmup, a.reps)
            rec.update({'torch_ops_us': round(t_med, 1), 'torch_ops_min_us': round(t_min, 1), 'torch_ops_max_us': round(t_max, 1),
                        'torch_over_ours': round(t_med / o_med, 2)})
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=550)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--skip-torch', action='store_true')
    ap.add_argument('--step', choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    if a.step is None:
        # one fresh process per step, each under its own time limit; a step that fails ends the probe
        for step, limit in STEPS:
            cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', step, '--batch', str(a.batch),
                   '--size', str(a.size), '--reps', str(a.reps), '--warmup', str(a.warmup)] + (['--skip-torch'] if a.skip_torch else [])
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print('step %s ended with status %d: the probe stops here' % (step, rc), flush=True)
                return rc
        return 0
    import torch
    sys.path.insert(0, ROOT)
    from yolact_amd import _lib as L
    from yolact_amd.layers import train_ops as TO
    if not torch.cuda.is_available():
        raise SystemExit('stem_train_probe: no GPU; a time is measured on the MI355X or not at all')
    print('step %s on %s, torch %s' % (a.step, torch.cuda.get_device_name(0), torch.__version__), flush=True)
    {'calib': step_calib, 'wgrad': step_wgrad, 'pool': step_pool, 'stem': step_stem}[a.step](a, torch, L, TO)
    return 0


if __name__ == '__main__':
    sys.exit(main())
