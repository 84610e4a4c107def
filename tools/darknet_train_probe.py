#!/usr/bin/env python3
"""Time the train-mode DarkNet53 backbone (train_net.darknet; csrc/bn_train.hip ymi_bn_leaky_*, csrc/darknet_train.hip) at B = 8 on
550 x 550 images, each against the PyTorch composition on the same GPU in the same run:

  calib   ymi_calib_hbm_copy over 1 GiB, as bench.py's box calibration times it: the memory bandwidth every byte count below is set
          against (the README quotes 6.29 TB/s for it).
  wgrad   ymi_preconv_wgrad_nhwc_f32 (x [8,550,550,4], g [8,550,550,32]) against torch.nn.grad.conv2d_weight on the NCHW image, and the
          time of ONE pass over its g and x bytes at the calibrated bandwidth.
  bn      ymi_bn_leaky_fwd_nhwc_f32 and ymi_bn_leaky_bwd_nhwc_f32 alone on [8*550*550, 32] (the pre-convolution's map) and [8*18*18, 1024]
          (the last stage's), batch statistics and frozen, without and with the residual, and the bytes/s each pass achieves over the maps
          its kernels read and write.
  step    forward + backward of train_net.darknet on yolact_darknet53's backbone with a gradient into every stage output, frozen and
          batch statistics, the device time of every entry point summed per kernel family (events around each call of the library),
          against the same backbone composed of torch.nn modules (Conv2d, BatchNorm2d, LeakyReLU on NCHW tensors) with autograd.

HIP events around each call, WARMUP warm-ups, the median and the least of REPS.  One JSON line per measurement.  Without --step every
step runs in a process of its own under its own time limit (`timeout`), one after the other; the first step that fails or runs out of
time ends the probe, and nothing more is started on the GPU.

    python tools/darknet_train_probe.py [--batch 8] [--size 550] [--reps 10] [--warmup 3] [--skip-torch] [--step calib|wgrad|bn|step]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

STEPS = (('calib', 120), ('wgrad', 180), ('bn', 240), ('step', 420))        # (step, its time limit in seconds)
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
    dev, B, S, Cout = 'cuda:0', a.batch, a.size, 32
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, S, S, generator=gen).to(dev)
    x4 = F.pad(x.permute(0, 2, 3, 1), (0, 1)).contiguous()
    g = torch.randn(B, S, S, Cout, generator=gen).to(dev)
    dw = torch.empty(27, Cout, device=dev)
    lib, s = L.lib(), L.stream_ptr()
    d = L.PreconvWgradDesc()
    d.x, d.g, d.dw = x4.data_ptr(), g.data_ptr(), dw.data_ptr()
    d.B, d.H, d.W, d.Cout, d.ldg = B, S, S, Cout, Cout
    nbytes = lib.ymi_workspace_bytes(L.WS_PRECONV_WGRAD, C.byref(d))
    assert nbytes > 0, nbytes
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    d.ws, d.ws_bytes = ws.data_ptr(), int(nbytes)

    def kernel():
        rc = lib.ymi_preconv_wgrad_nhwc_f32(C.byref(d), s)
        assert rc == 0, rc
    k_med, k_min, _ = timed(torch, kernel, a.warmup, a.reps)
    gbps, _ = hbm_gbps(torch, L)
    nb = 4.0 * (g.numel() + x4.numel())
    flops = 2.0 * B * S * S * 27 * Cout
    rec = {'probe': 'preconv wgrad 3x3 / stride 1, 3 -> %d at %d x %d^2' % (Cout, B, S), 'kernel_us': round(k_med, 1),
           'kernel_min_us': round(k_min, 1), 'kernel_tflops_useful': round(flops / k_med * 1e-6, 2), 'workspace_MB': round(nbytes / 2 ** 20, 1),
           'g_plus_x_MB': round(nb / 2 ** 20, 1), 'kernel_GBps': round(nb / k_med * 1e-3, 1), 'hbm_copy_GBps': round(gbps, 1),
           'one_pass_over_g_and_x_us': round(nb / gbps * 1e-3, 1), 'kernel_over_one_pass': round(k_med / (nb / gbps * 1e-3), 2)}
    if not a.skip_torch:
        gn = g.permute(0, 3, 1, 2)
        ref = torch.nn.grad.conv2d_weight(x, (Cout, 3, 3, 3), gn, stride=1, padding=1)
        kernel()
        torch.cuda.synchronize()
        rec['max_rel_difference'] = float((TO._unpack_dw(dw, 3, 3) - ref).abs().max() / ref.abs().max())
        t_med, t_min, _ = timed(torch, lambda: torch.nn.grad.conv2d_weight(x, (Cout, 3, 3, 3), gn, stride=1, padding=1), a.warmup, a.reps)
        rec.update({'torch_conv2d_weight_us': round(t_med, 1), 'torch_min_us': round(t_min, 1), 'torch_over_ours': round(t_med / k_med, 2)})
    print(json.dumps(rec), flush=True)


def step_bn(a, torch, L, TO):
    import torch.nn.functional as F
    dev = 'cuda:0'
    lib, s = L.lib(), L.stream_ptr()
    gbps, _ = hbm_gbps(torch, L)
    last = a.size
    for _ in range(5):
        last = (last - 1) // 2 + 1
    for npos, Cc in ((a.batch * a.size * a.size, 32), (a.batch * last * last, 1024)):
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(npos, Cc, generator=gen).to(dev)
        res, dy = torch.randn(npos, Cc, generator=gen).to(dev), torch.randn(npos, Cc, generator=gen).to(dev)
        gamma, beta = (0.5 + torch.rand(Cc, generator=gen)).to(dev), (torch.randn(Cc, generator=gen) * 0.1).to(dev)
        rm, rv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, invstd, dg, db = (torch.empty(Cc, device=dev) for _ in range(4))
        mask = torch.empty((npos * Cc + 31) // 32, dtype=torch.int32, device=dev)
        for training in (1, 0):
            for residual in (False, True):
                d = L.BnDesc()
                d.x, d.gamma, d.beta, d.res = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), (res.data_ptr() if residual else None)
                d.running_mean, d.running_var, d.y, d.mean, d.invstd = rm.data_ptr(), rv.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr()
                d.dy, d.dx, d.dgamma, d.dbeta = dy.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr()
                d.npos, d.C, d.training, d.relu, d.eps, d.momentum = npos, Cc, training, 0, 1e-5, 0.1
                nbytes = lib.ymi_workspace_bytes(L.WS_BN, C.byref(d))
                ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
                d.ws, d.ws_bytes = ws.data_ptr(), int(nbytes)
                mp = mask.data_ptr() if residual else None

                def fwd():
                    rc = lib.ymi_bn_leaky_fwd_nhwc_f32(C.byref(d), mp, s)
                    assert rc == 0, rc

                def bwd():
                    rc = lib.ymi_bn_leaky_bwd_nhwc_f32(C.byref(d), mp, s)
                    assert rc == 0, rc
                f_med, f_min, _ = timed(torch, fwd, a.warmup, a.reps)
                b_med, b_min, _ = timed(torch, bwd, a.warmup, a.reps)
                m = 4.0 * npos * Cc                                  # one map
                # forward: x once per statistics pass (two) and once in the apply, y written, the residual read, the mask written
                fb = m * ((3 if training else 1) + 1 + (1 + 1 / 32 if residual else 0))
                # backward: the sums read dy, x and the decisions (y, or the mask); the apply reads dy, the decisions (and x with the
                # batch statistics) and writes dx
                dec = 1 / 32 if residual else 1
                bb = m * ((2 + dec) + (1 + dec + (1 if training else 0)) + 1)
                rec = {'probe': 'leaky BN alone, [%d, %d], %s%s' % (npos, Cc, 'batch statistics' if training else 'frozen',
                                                                   ', residual' if residual else ''),
                       'fwd_us': round(f_med, 1), 'fwd_min_us': round(f_min, 1), 'fwd_GBps': round(fb / f_med * 1e-3, 1),
                       'bwd_us': round(b_med, 1), 'bwd_min_us': round(b_min, 1), 'bwd_GBps': round(bb / b_med * 1e-3, 1),
                       'map_MB': round(m / 2 ** 20, 1), 'hbm_copy_GBps': round(gbps, 1),
                       'fwd_share_of_copy': round(fb / f_med * 1e-3 / gbps, 2), 'bwd_share_of_copy': round(bb / b_med * 1e-3 / gbps, 2)}
                if not a.skip_torch:
                    xn = x.t().reshape(1, Cc, npos, 1).requires_grad_(True)
                    gl, bl = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
                    rn, dn = res.t().reshape(1, Cc, npos, 1), dy.t().reshape(1, Cc, npos, 1)

                    def t_fwd():
                        z = F.leaky_relu(F.batch_norm(xn, rm.clone(), rv.clone(), gl, bl, bool(training), 0.1, 1e-5), 0.1)
                        return z + rn if residual else z
                    out = t_fwd()
                    tf_med, _, _ = timed(torch, lambda: t_fwd(), a.warmup, a.reps)
                    tb_med, _, _ = timed(torch, lambda: torch.autograd.grad(out, [xn, gl, bl], dn, retain_graph=True), a.warmup, a.reps)
                    rec.update({'torch_fwd_us': round(tf_med, 1), 'torch_bwd_us': round(tb_med, 1),
                                'torch_over_ours': round((tf_med + tb_med) / (f_med + b_med), 2)})
                print(json.dumps(rec), flush=True)


FAMILIES = {'ymi_conv2d_nhwc_f32': 'conv forward and stride-1 dx (engine)', 'ymi_conv_wgrad_nhwc_f32': 'conv wgrad',
            'ymi_conv_dgrad_s2_nhwc_f32': 'conv stride-2 dx', 'ymi_bn_leaky_fwd_nhwc_f32': 'leaky BN forward',
            'ymi_bn_leaky_bwd_nhwc_f32': 'leaky BN backward', 'ymi_preconv_wgrad_nhwc_f32': 'preconv wgrad'}


class TimedLib:
    """The library with HIP events around every call of the entries in FAMILIES."""

    def __init__(self, torch, lib):
        self.torch, self.lib, self.on, self.events = torch, lib, False, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in FAMILIES:
            return fn

        def call(*args):
            if not self.on:
                return fn(*args)
            a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            self.events.append((name, a, b))
            return rc
        return call

    def totals(self, runs):
        """After a synchronise: microseconds per family and run."""
        out = {}
        for name, a, b in self.events:
            out[FAMILIES[name]] = out.get(FAMILIES[name], 0.0) + a.elapsed_time(b) * 1e3 / runs
        self.events = []
        return {k: round(v, 1) for k, v in out.items()}


def step_step(a, torch, L, TO):
    import types
    from yolact_amd import modules as M
    from yolact_amd import train_net as TN
    dev = 'cuda:0'
    torch.manual_seed(0)
    bb = M.DarkNetBackbone().to(dev)
    holder = types.SimpleNamespace(backbone=bb)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(a.batch, 3, a.size, a.size, generator=gen).to(dev)
    plist = list(bb.parameters())
    with torch.no_grad():
        ups = [torch.randn(*o.shape, generator=gen).to(dev) for o in TN.darknet(holder, x, False)]
    proxy = TimedLib(torch, L.lib())
    L.lib = lambda: proxy
    for batch_stats in (False, True):
        def clear():
            for t in plist:
                t.grad = None

        def ours():
            clear()
            sum((o * u).sum() for o, u in zip(TN.darknet(holder, x, batch_stats), ups)).backward()

        def ours_fwd():
            with torch.no_grad():
                TN.darknet(holder, x, batch_stats)

        def torch_ops():
            clear()
            bb.train(batch_stats)
            h, tot = bb._preconv(x), 0.0
            for layer, u in zip(bb.layers, ups):
                h = layer[0](h)
                for blk in list(layer)[1:]:
                    h = blk.conv2(blk.conv1(h)) + h
                tot = tot + (h * u.permute(0, 3, 1, 2)).sum()
            tot.backward()
            bb.eval()
        o_med, o_min, o_max = timed(torch, ours, a.warmup, a.reps)
        proxy.on = True
        for _ in range(3):
            ours()
        torch.cuda.synchronize()
        fam = proxy.totals(3)
        proxy.on = False
        rec = {'probe': 'train_net.darknet forward + backward, DarkNet53, B %d, %d x %d, %s' % (a.batch, a.size, a.size,
                                                                                              'batch statistics' if batch_stats else 'frozen BN'),
               'ours_us': round(o_med, 1), 'ours_min_us': round(o_min, 1), 'ours_max_us': round(o_max, 1),
               'ours_forward_only_us': round(timed(torch, ours_fwd, a.warmup, a.reps)[0], 1), 'entry_points_us': fam,
               'entry_points_sum_us': round(sum(fam.values()), 1)}
        if not a.skip_torch:
            t_med, t_min, t_max = timed(torch, torch_ops, a.warmup, a.reps)
            rec.update({'torch_nn_us': round(t_med, 1), 'torch_nn_min_us': round(t_min, 1), 'torch_nn_max_us': round(t_max, 1),
                        'torch_over_ours': round(t_med / o_med, 2)})
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=550)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
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
        raise SystemExit('darknet_train_probe: no GPU; a time is measured on the MI355X or not at all')
    print('step %s on %s, torch %s' % (a.step, torch.cuda.get_device_name(0), torch.__version__), flush=True)
    {'calib': step_calib, 'wgrad': step_wgrad, 'bn': step_bn, 'step': step_step}[a.step](a, torch, L, TO)
    return 0


if __name__ == '__main__':
    sys.exit(main())
