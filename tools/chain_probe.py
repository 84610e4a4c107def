#!/usr/bin/env python
"""ymi_pointwise_chain_f32 (csrc/chain.hip) at the shape it exists for: the first ResNet stage at 138 x 138 x batch.

    python tools/chain_probe.py [--batch 8] [--reps 10] [--sets 3]

Times the launch in its three forms (conv3 + residual -> conv1; without the second layer; without the residual) on `--sets`
rotating buffer sets (3 x 390 MB: nothing survives in the 256 MB memory-side cache between launches, like in a real step, where
the operands were written by the previous layer and everything else has passed through since), and prints the bytes per second of
the launch's algorithmic traffic.  The two launches of the plan it replaces: layer0.N.conv3 0.083 + layer0.(N+1).conv1 0.055 ms
in the step (profiles/r04_layers.txt), 0.0745 + 0.035 ms alone on resident buffers (profiles/r04_ws_probe.txt).

Then the stage EXIT (ymi_stage_exit_chain_f32: layer0.2.conv3 + residual -> layer1.0.conv1, 256 -> 128, y stored at even rows and
columns only) next to the two launches it replaces: the chain kernel without its second layer ('chain1') and the plan's 1x1
256 -> 128 convolution on the tile the shipped table gives that shape; same rotating buffer sets.

Then the stage ENTRY (ymi_chain_desc.x0: layer0.0's projection shortcut computed inside the layer0.0.conv3 -> layer0.1.conv1 launch):
the shortcut launch alone on its shipped tile, the shortcut launch followed by the pair chain, and the entry launch; same sets.
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sets', type=int, default=3)
    args = ap.parse_args()
    from yolact_amd import _lib as L
    from yolact_amd.engine import Packed
    dev = torch.device('cuda', 0)
    M = args.batch * 138 * 138
    g = torch.Generator().manual_seed(1)
    wa = torch.randn(256, 64, 1, 1, generator=g) / 8
    wb = torch.randn(64, 256, 1, 1, generator=g) / 16
    pa, pb = Packed(wa, torch.randn(256, generator=g), None, 1, 0, None, dev), Packed(wb, torch.randn(64, generator=g), None, 1, 0, None, dev)
    pla, sca, _ = pa.h2()
    plb, scb, _ = pb.h2()
    sets = []
    for _ in range(args.sets):
        x = torch.randn(M, 64, device=dev).relu_()
        res = torch.randn(M, 256, device=dev).relu_()
        sets.append((x, res, torch.empty(M, 256, device=dev), torch.empty(M, 64, device=dev)))
    amax = torch.zeros(5 * 1024, device=dev)
    lib, s = L.lib(), L.stream_ptr()
    L.check(lib.ymi_amax_f32(sets[0][0].data_ptr(), sets[0][0].numel(), amax.data_ptr(), s))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def desc(k, two, with_res):
        x, res, y, z = sets[k]
        d = L.ChainDesc()
        d.x, d.y, d.M, d.ldx, d.ldy = x.data_ptr(), y.data_ptr(), M, 64, 256
        d.w_a_h2, d.scale_a_h2, d.bias_a, d.cout_pad_a = pla.data_ptr(), sca.data_ptr(), pa.bias.data_ptr(), pa.CoutPad
        d.k_a, d.n_a, d.n_b, d.act_a, d.act_b = 64, 256, 64, L.ACT_RELU, L.ACT_RELU
        d.x_amax, d.y_amax, d.z_amax = amax.data_ptr(), amax.data_ptr() + 4096, amax.data_ptr() + 8192
        if with_res:
            d.res, d.res_ld = res.data_ptr(), 256
        if two:
            d.z, d.ldz, d.w_b_h2, d.scale_b_h2, d.bias_b, d.cout_pad_b = z.data_ptr(), 64, plb.data_ptr(), scb.data_ptr(), pb.bias.data_ptr(), pb.CoutPad
        return d
    for name, two, with_res in (('conv3 + residual -> conv1', True, True), ('conv3 + residual', False, True), ('conv3 -> conv1, no residual', True, False)):
        ds = [desc(k, two, with_res) for k in range(args.sets)]
        for d in ds:
            L.check(lib.ymi_pointwise_chain_f32(C.byref(d), s))
        best = 1e30
        for _ in range(3):
            e0.record()
            for r in range(args.reps):
                lib.ymi_pointwise_chain_f32(C.byref(ds[r % args.sets]), s)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / args.reps)
        nbytes = 4.0 * M * (64 + 256 + (256 if with_res else 0) + (64 if two else 0))
        print('%-30s M=%d  %.4f ms  %6.1f MB  %.2f TB/s' % (name, M, best, nbytes / 1e6, nbytes / best / 1e9))

    # ---- the stage exit against the two launches it replaces
    from yolact_amd import tune_table as TT
    B, H, W = args.batch, 138, 138
    wx = torch.randn(128, 256, 1, 1, generator=g) / 16
    px = Packed(wx, torch.randn(128, generator=g), None, 1, 0, None, dev)
    plx, scx, winvx = px.h2()
    zs = [torch.empty(M, 128, device=dev) for _ in range(args.sets)]

    def conv1_desc(k):
        d = L.ConvDesc()
        d.x, d.w, d.bias = sets[k][2].data_ptr(), px.w.data_ptr(), px.bias.data_ptr()
        d.scale = px.scale.data_ptr() if px.scale is not None else None
        d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = B, H, W, 256, 256, H, W, 128
        d.kh, d.kw, d.stride, d.pad, d.Kpad, d.cin_alg, d.cout_alg = 1, 1, 1, 0, px.Kpad, px.cin_alg, px.cout_alg
        d.nseg = 1
        d.seg[0] = L.ConvSeg(0, 128, L.ACT_RELU, 128, H * W * 128, zs[k].data_ptr())
        d.x_amax, d.y_amax = amax.data_ptr() + 4096, amax.data_ptr() + 8192
        d.w_h2, d.scale_h2, d.winv_h2 = plx.data_ptr(), scx.data_ptr(), winvx.data_ptr()
        val = TT.load_tune_table(dev).get(TT.conv_key((B, H, W, 256, 128, 1, 1, 1, 0, 0, 1, 256), 'h2'))
        d.tile = TT.direct_parts(val)[0] if val is not None else L.TILE_AUTO
        return d

    def exit_desc(k, y_stride):
        e = L.StageExitDesc()
        e.chain = desc(k, False, True)           # (a copy: conv3 + residual as in the arms above)
        c = e.chain
        c.n_b, c.z, c.ldz, c.z_amax = 128, zs[k].data_ptr(), 128, amax.data_ptr() + 8192
        c.w_b_h2, c.scale_b_h2, c.bias_b, c.cout_pad_b = plx.data_ptr(), scx.data_ptr(), px.bias.data_ptr(), px.CoutPad
        e.B, e.H, e.W, e.y_stride = B, H, W, y_stride
        return e
    c3 = [desc(k, False, True) for k in range(args.sets)]
    c1 = [conv1_desc(k) for k in range(args.sets)]
    arms = [('chain1 (conv3 + residual)', lambda k: lib.ymi_pointwise_chain_f32(C.byref(c3[k]), s), 4.0 * M * (64 + 256 + 256)),
            ('layer1.0.conv1 (tile %d)' % c1[0].tile, lambda k: lib.ymi_conv2d_nhwc_f32(C.byref(c1[k]), s), 4.0 * M * (256 + 128)),
            ('chain1, then conv1', lambda k: (lib.ymi_pointwise_chain_f32(C.byref(c3[k]), s), lib.ymi_conv2d_nhwc_f32(C.byref(c1[k]), s))[1],
             4.0 * M * (64 + 256 + 256 + 256 + 128))]
    for ys in (2, 1):
        xs = [exit_desc(k, ys) for k in range(args.sets)]
        arms.append(('stage exit, y_stride %d' % ys, (lambda k, xs=xs: lib.ymi_stage_exit_chain_f32(C.byref(xs[k]), s)),
                     4.0 * M * (64 + 256 + 128) + 4.0 * B * ((H + ys - 1) // ys) * ((W + ys - 1) // ys) * 256))
    for name, run, nbytes in arms:
        for k in range(args.sets):
            L.check(run(k))
        best = 1e30
        for _ in range(3):
            e0.record()
            for r in range(args.reps):
                run(r % args.sets)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / args.reps)
        print('%-30s M=%d  %.4f ms  %6.1f MB  %.2f TB/s' % (name, M, best, nbytes / 1e6, nbytes / best / 1e9))

    # ---- the stage ENTRY: layer0.0's projection shortcut (1x1, 64 -> 256, no activation) on the tile the shipped table gives it, that
    # launch followed by the pair chain that reads its output as the residual, and the entry launch that computes it inside
    wd = torch.randn(256, 64, 1, 1, generator=g) / 8
    pd = Packed(wd, torch.randn(256, generator=g), None, 1, 0, None, dev)
    pld, scd, winvd = pd.h2()
    x0s = [torch.randn(M, 64, device=dev).relu_() for _ in range(args.sets)]
    L.check(lib.ymi_amax_f32(x0s[0].data_ptr(), x0s[0].numel(), amax.data_ptr() + 12288, s))

    def down_desc(k):
        d = L.ConvDesc()
        d.x, d.w, d.bias = x0s[k].data_ptr(), pd.w.data_ptr(), pd.bias.data_ptr()
        d.scale = pd.scale.data_ptr() if pd.scale is not None else None
        d.B, d.H, d.W, d.Cin, d.ldx, d.Ho, d.Wo, d.Cout = B, H, W, 64, 64, H, W, 256
        d.kh, d.kw, d.stride, d.pad, d.Kpad, d.cin_alg, d.cout_alg = 1, 1, 1, 0, pd.Kpad, pd.cin_alg, pd.cout_alg
        d.nseg = 1
        d.seg[0] = L.ConvSeg(0, 256, L.ACT_NONE, 256, H * W * 256, sets[k][1].data_ptr())      # (into the set's residual tensor)
        d.x_amax, d.y_amax = amax.data_ptr() + 12288, amax.data_ptr() + 16384
        d.w_h2, d.scale_h2, d.winv_h2 = pld.data_ptr(), scd.data_ptr(), winvd.data_ptr()
        val = TT.load_tune_table(dev).get(TT.conv_key((B, H, W, 64, 256, 1, 1, 1, 0, 0, 1, 64), 'h2'))
        d.tile = TT.direct_parts(val)[0] if val is not None else L.TILE_AUTO
        return d

    def entry_desc(k):
        d = desc(k, True, False)
        d.x0, d.ldx0, d.x0_amax = x0s[k].data_ptr(), 64, amax.data_ptr() + 12288
        d.w_d_h2, d.scale_d_h2, d.bias_d, d.cout_pad_d = pld.data_ptr(), scd.data_ptr(), pd.bias.data_ptr(), pd.CoutPad
        return d
    dn = [down_desc(k) for k in range(args.sets)]
    pair = [desc(k, True, True) for k in range(args.sets)]
    ent = [entry_desc(k) for k in range(args.sets)]
    arms = [('layer0.0.down (tile %d)' % dn[0].tile, lambda k: lib.ymi_conv2d_nhwc_f32(C.byref(dn[k]), s), 4.0 * M * (64 + 256)),
            ('down, then pair chain', lambda k: (lib.ymi_conv2d_nhwc_f32(C.byref(dn[k]), s), lib.ymi_pointwise_chain_f32(C.byref(pair[k]), s))[1],
             4.0 * M * (64 + 256 + 64 + 256 + 256 + 64)),
            ('entry chain (down inside)', lambda k: lib.ymi_pointwise_chain_f32(C.byref(ent[k]), s), 4.0 * M * (64 + 64 + 256 + 64))]
    for name, run, nbytes in arms:
        for k in range(args.sets):
            L.check(run(k))
        best = 1e30
        for _ in range(3):
            e0.record()
            for r in range(args.reps):
                run(r % args.sets)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / args.reps)
        print('%-30s M=%d  %.4f ms  %6.1f MB  %.2f TB/s' % (name, M, best, nbytes / 1e6, nbytes / best / 1e9))


if __name__ == '__main__':
    main()
