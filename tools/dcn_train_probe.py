#!/usr/bin/env python3
"""Time train_ops.deform_conv (csrc/dcn_train.hip + the Conv function) on the six YOLACT++ DCN shapes at batch 8, next to the only
other differentiable route in the tree, dcn_v2.dcn_v2_conv (NCHW, host-packed filters, fp32 atomics, csrc/dcn_bwd.hip), on the same data.

Per shape: forward, and forward + backward (all gradients), of both routes, HIP events around each, WARMUP warm-ups, the median of REPS
(and the minimum); then the pieces of the new backward on their own, each as a share of the sum of the pieces: the GEMM half
(Conv's backward: ymi_act_bwd_f32, ymi_conv_wgrad_nhwc_f32, the data gradient on the engine -> dcol), ymi_dcn_cols_entries_f32, the stable
torch.sort of the keys, the g_om launch and the gx launches (segment starts + gather) of ymi_dcn_cols_bwd_f32; and the bytes of col.
The atomic route's time includes its NCHW <-> NHWC changes: that is what a caller of it pays.  Recorded, not gated.

    python tools/dcn_train_probe.py [--batch 8] [--reps 20] [--warmup 5] [--out profiles/dcn_train_probe_b8.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import dcn_v2  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

SHAPES = [(128, 138, 2), (128, 69, 1), (256, 69, 2), (256, 35, 1), (512, 35, 2), (512, 18, 1)]        # Cin = Cout, input size, stride


def timed(fn, warmup, reps):
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
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe measures on the GPU; there is nothing to report without one'
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    lines = ['device: %s  torch %s  batch %d  reps %d (median, us)' % (torch.cuda.get_device_name(0), torch.__version__, a.batch, a.reps)]
    print(lines[0])
    for Cc, S, stride in SHAPES:
        B = a.batch
        So = (S - 1) // stride + 1
        x = torch.randn(B, S, S, Cc, generator=g).to(dev)
        w = (torch.randn(Cc, Cc, 3, 3, generator=g) * (2.0 / (9 * Cc)) ** 0.5).to(dev)
        bias = torch.randn(Cc, generator=g).to(dev)
        om = torch.cat([torch.randn(B, So, So, 18, generator=g) * 2, torch.randn(B, So, So, 9, generator=g)], 3).to(dev)
        gy = torch.randn(B, So, So, Cc, generator=g).to(dev)
        leaves = [t.clone().requires_grad_(True) for t in (x, om, w, bias)]

        def new_fwd():
            with torch.no_grad():
                return TO.deform_conv(x, om, w, bias, stride)

        def new_both():
            for t in leaves:
                t.grad = None
            TO.deform_conv(*leaves, stride).backward(gy)

        # the atomic route on the same data, as its callers reach it: NCHW tensors, the modulation passed in
        xn, gyn = x.permute(0, 3, 1, 2).contiguous(), gy.permute(0, 3, 1, 2).contiguous()
        omn = om.permute(0, 3, 1, 2).contiguous()
        old_leaves = [t.clone().requires_grad_(True) for t in (xn, omn, w, bias)]

        def old_fwd():
            with torch.no_grad():
                return dcn_v2.dcn_v2_conv(xn, omn[:, :18], torch.sigmoid(omn[:, 18:]), w, bias, stride, 1, 1, 1)

        def old_both():
            for t in old_leaves:
                t.grad = None
            o = old_leaves[1]
            dcn_v2.dcn_v2_conv(old_leaves[0], o[:, :18], torch.sigmoid(o[:, 18:]), old_leaves[2], old_leaves[3], stride, 1, 1, 1).backward(gyn)

        # the two routes compute the same thing (fp32-class)
        y_new, y_old = new_fwd(), old_fwd().permute(0, 2, 3, 1)
        agree = ((y_new - y_old).abs().max() / y_old.abs().max()).item()

        # the pieces of the new backward
        col = TO.DeformCols.apply(stride, x, om)
        col_leaf = col.clone().requires_grad_(True)
        w1 = w.permute(0, 2, 3, 1).reshape(Cc, 9 * Cc, 1, 1).clone().requires_grad_(True)
        bl = bias.clone().requires_grad_(True)

        def gemm_bwd():
            for t in (col_leaf, w1, bl):
                t.grad = None
            TO.Conv.apply(1, 0, 1, (L.ACT_NONE,), False, col_leaf, w1, bl)[0].backward(gy)

        def gemm_fwd():
            with torch.no_grad():
                TO.Conv.apply(1, 0, 1, (L.ACT_NONE,), False, col, w1, bl)

        dcol = torch.randn(B, So, So, 9 * Cc, generator=g).to(dev)
        d, _, _ = TO._cols_desc(x, om, stride)
        n = 36 * B * So * So
        keys, coef = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        seg, gx, g_om = torch.empty(B * S * S + 1, dtype=torch.int32, device=dev), torch.empty_like(x), torch.empty_like(om)
        d.dcol, d.keys, d.coef, d.col = dcol.data_ptr(), keys.data_ptr(), coef.data_ptr(), col.data_ptr()
        entries = lambda: L.check(L.lib().ymi_dcn_cols_entries_f32(C.byref(d), L.stream_ptr()), 'entries')
        entries()
        skeys, order = torch.sort(keys, stable=True)
        d_om, _, _ = TO._cols_desc(x, om, stride)
        d_om.dcol, d_om.g_om = dcol.data_ptr(), g_om.data_ptr()
        d_gx, _, _ = TO._cols_desc(x, om, stride)
        d_gx.dcol, d_gx.gx, d_gx.coef, d_gx.seg = dcol.data_ptr(), gx.data_ptr(), coef.data_ptr(), seg.data_ptr()
        d_gx.sorted_keys, d_gx.order = skeys.data_ptr(), order.data_ptr()
        bwd = lambda dd: (lambda: L.check(L.lib().ymi_dcn_cols_bwd_f32(C.byref(dd), L.stream_ptr()), 'cols bwd'))
        cols_fwd = lambda: L.check(L.lib().ymi_dcn_cols_fwd_f32(C.byref(d), L.stream_ptr()), 'cols fwd')

        t = lambda fn: timed(fn, a.warmup, a.reps)
        (nf, _), (nb, nb_min), (of, _), (ob, ob_min) = t(new_fwd), t(new_both), t(old_fwd), t(old_both)
        pieces = {'gemm_fwd_plus_bwd': t(gemm_bwd)[0], 'gemm_fwd': t(gemm_fwd)[0], 'cols_fwd': t(cols_fwd)[0], 'entries': t(entries)[0],
                  'sort': t(lambda: torch.sort(keys, stable=True))[0], 'g_om': t(bwd(d_om))[0], 'gx_seg_plus_gather': t(bwd(d_gx))[0]}
        gemm_b = pieces['gemm_fwd_plus_bwd'] - pieces['gemm_fwd']
        back = {'gemm_bwd': gemm_b, 'entries': pieces['entries'], 'sort': pieces['sort'], 'g_om': pieces['g_om'],
                'gx_seg_plus_gather': pieces['gx_seg_plus_gather']}
        tot = sum(back.values())
        lens = torch.bincount(skeys[skeys < B * S * S].long(), minlength=B * S * S)
        rec = {'shape': 'B%d c%d %dx%d s%d' % (B, Cc, S, S, stride), 'col_MB': round(col.numel() * 4 / 1e6, 1),
               'new_forward_us': round(nf, 1), 'new_fwd_bwd_us': round(nb, 1), 'new_fwd_bwd_min_us': round(nb_min, 1),
               'atomic_forward_us': round(of, 1), 'atomic_fwd_bwd_us': round(ob, 1), 'atomic_fwd_bwd_min_us': round(ob_min, 1),
               'new_over_atomic_fwd_bwd': round(nb / ob, 2), 'forward_pieces_us': {'cols_fwd': round(pieces['cols_fwd'], 1),
                                                                                    'gemm_fwd': round(pieces['gemm_fwd'], 1)},
               'backward_pieces_us': {k: round(v, 1) for k, v in back.items()},
               'backward_shares': {k: round(v / tot, 3) for k, v in back.items()},
               'gx_list_len_median_max': [int(lens.median()), int(lens.max())], 'forward_rel_diff_new_vs_atomic': float('%.2e' % agree)}
        lines.append(json.dumps(rec))
        print(lines[-1])
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
