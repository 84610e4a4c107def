#!/usr/bin/env python3
"""One SHA-256 per output tensor of the train-mode building blocks (yolact_amd/layers/train_ops.py) on fixed inputs: two trees whose
lines are equal issue the same launches on the same operands.  Only public functions are called (conv2d_act, conv2d_multi,
conv2d_down, conv2d_plain, bottleneck, upsample2x, upsample_add, batch_norm_act, stem_conv, max_pool_3x3_s2 and Yolact.forward_stem /
forward_backbone / forward_fpn / forward_heads / forward_train), so the script runs unchanged on an older tree.  The shapes are the
small ones of tests/test_gpu_heads_train.py, tests/test_gpu_fpn_train.py and tests/test_gpu_backbone_train.py; the inputs come from
seeded CPU generators.  Per case: y and every gradient (for a bottleneck the running statistics afterwards too).  The net-level cases
run on the model of tests/test_gpu_stem_train.py::test_multibox_loss_from_the_images (seeded ResNet-50 stages, 32 features, 96 x 96
images) with random inputs: every output and every parameter gradient, with frozen and with batch statistics.  The weight-gradient
entries ymi_conv_wgrad_nhwc_f32 and ymi_stem_wgrad_nhwc_f32 are also called on their own (WGRAD_SHAPES, STEM_WGRAD_SHAPES) at the edges
of their position walk and chunk plan; the C ABI they are called through is that of every tree with these entries.
fold_cases() reaches what the older cases leave out, through public functions too: batch_norm_leaky and batch_norm_act where only the
residual asks for a gradient, preconv, dark_unit, dark_block, deform_conv, dcn_bottleneck, the convolutions under conv_mode / wgrad_mode
with the backward inside and behind the `with`, and train_net.forward on a DarkNet of one block per stage.

    python tools/train_digest.py > digests.txt
    python tools/train_digest.py --per-case > digests.txt      one line per case: its number of tensor lines and the SHA-256 of them
"""
import contextlib
import ctypes as C
import hashlib
import math
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import backbone_train_ref as R  # noqa: E402
import heads_train_ref as H  # noqa: E402
import yolact_amd  # noqa: E402, F401
from yolact_amd import _lib as L  # noqa: E402
from yolact_amd import modules as M  # noqa: E402
from yolact_amd import train_net as TN  # noqa: E402
from yolact_amd.layers import train_ops as TO  # noqa: E402

DEV = 'cuda:0'
ACT_SHAPES = [(3, 2, 5, 7, 32, 12), (3, 1, 9, 9, 64, 243), (1, 3, 6, 6, 256, 32)]            # (k, B, H, W, Cin, Cout)
DOWN_SHAPES = [(3, 2, 5, 7, 32, 12), (3, 1, 8, 6, 64, 40), (1, 2, 7, 9, 64, 32)]
PLAIN_GEOS = [(3, 1, 32, 40), (1, 1, 64, 32), (3, 2, 32, 32), (1, 2, 64, 96), (3, 2, 64, 40)]   # (k, stride, Cin, Cout) at B = 2, 9 x 7
BLOCK_SPECS = {'identity': (128, 32, 1, False), 'proj_s1': (64, 32, 1, True), 'proj_s2': (64, 32, 2, True), 'entry': (64, 64, 1, True)}
ACTS = (None, 'relu', 'tanh')
# (k, stride, B, H, W, Cin, Cout): a map one pixel wide (the walk wraps twice per step) at both strides; 1 058 positions in 12 chunks of 96,
# the last of 2; two and four column tiles per wave at stride 2
WGRAD_SHAPES = [(3, 1, 3, 5, 1, 32, 32), (3, 2, 3, 5, 1, 32, 32), (3, 1, 2, 23, 23, 256, 32), (3, 2, 2, 5, 7, 32, 160),
                (3, 2, 2, 5, 7, 32, 288)]
STEM_WGRAD_SHAPES = [(1, 9, 9, 32)]                                                            # (B, H, W, Cout)


PER_CASE = None            # --per-case: case -> its tensor lines, kept back and hashed at the end


def emit(case, name, t):
    t = t.detach().cpu().contiguous()
    line = '%-30s %-26s %-7s %-18s %s' % (case, name, str(t.dtype)[6:], list(t.shape), hashlib.sha256(t.numpy().tobytes()).hexdigest())
    if PER_CASE is None:
        print(line)
    else:
        PER_CASE.setdefault(case, []).append(line)


def leaf(t, grad=True, dtype=None):
    return t.to(device=DEV, dtype=dtype).requires_grad_(grad)


def backward_and_emit(case, ys, ups, leaves):
    """ys: the outputs that enter the loss (each with its upstream gradient); leaves: name -> tensor, those requiring grad are emitted."""
    sum((y * u.to(DEV)).sum() for y, u in zip(ys, ups)).backward()
    torch.cuda.synchronize()
    for n, t in leaves.items():
        if t.requires_grad:
            emit(case, 'd_' + n, t.grad)


def conv_inputs(g, k, B, H, W, Cin, Cout, Ho=None, Wo=None):
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    up = torch.randn(B, Ho or H, Wo or W, Cout, generator=g)
    return x, w, b, up


def act_case(case, shape, act, grads=(True, True, True), dtype=None):
    k = shape[0]
    x, w, b, up = conv_inputs(torch.Generator().manual_seed(5), *shape)
    leaves = dict(x=leaf(x, grads[0]), w=leaf(w, grads[1], dtype), b=leaf(b, grads[2], dtype))
    y = TO.conv2d_act(leaves['x'], leaves['w'], leaves['b'], k // 2, act)
    emit(case, 'y', y)
    backward_and_emit(case, [y], [up], leaves)


@contextlib.contextmanager
def under(modes):
    """modes None: nothing; (conv, wgrad): the two switches of train_ops around the block."""
    if modes is None:
        yield
    else:
        with TO.conv_mode(modes[0]), TO.wgrad_mode(modes[1]):
            yield


def forward_then_backward(case, modes, inside, forward, ups, leaves):
    """forward() -> outputs, under the modes; every output, then the gradients, from a backward inside the block or behind it."""
    def finish():
        for i, y in enumerate(ys):
            emit(case, 'y' if len(ys) == 1 else 'y%d' % i, y)
        backward_and_emit(case, ys[:len(ups)], ups, leaves)
    with under(modes):
        ys = forward()
        if inside:
            finish()
    if not inside:
        finish()


def multi_case(case, n_in_loss, modes=None, inside=True):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 5, 7, 32, generator=g)
    leaves, layers, ups = dict(x=leaf(x)), [], []
    for i, (co, act) in enumerate(zip((16, 81, 32), (None, None, 'tanh'))):
        _, w, b, up = conv_inputs(g, 3, 2, 5, 7, 32, co)
        leaves['w%d' % i], leaves['b%d' % i] = leaf(w), leaf(b)
        layers.append((leaves['w%d' % i], leaves['b%d' % i], act))
        ups.append(up)
    forward_then_backward(case, modes, inside, lambda: TO.conv2d_multi(leaves['x'], layers, 1), ups[:n_in_loss], leaves)


def down(n):
    return (n - 1) // 2 + 1


def down_case(case, shape, act, modes=None, inside=True):
    k, B, H, W, Cin, Cout = shape
    x, w, b, up = conv_inputs(torch.Generator().manual_seed(7), *shape, Ho=down(H), Wo=down(W))
    leaves = dict(x=leaf(x), w=leaf(w), b=leaf(b))
    forward_then_backward(case, modes, inside, lambda: [TO.conv2d_down(leaves['x'], leaves['w'], leaves['b'], act)], [up], leaves)


def plain_case(case, geo, modes=None, inside=True):
    k, stride, Cin, Cout = geo
    B, H, W = 2, 9, 7
    Ho, Wo = (down(H), down(W)) if stride == 2 else (H, W)
    x, w, _, up = conv_inputs(torch.Generator().manual_seed(8), k, B, H, W, Cin, Cout, Ho=Ho, Wo=Wo)
    leaves = dict(x=leaf(x), w=leaf(w))
    forward_then_backward(case, modes, inside, lambda: [TO.conv2d_plain(leaves['x'], leaves['w'], stride)], [up], leaves)


def block_case(case, spec, batch_stats):
    inplanes, planes, stride, projection = spec
    x, params, _, up = R.random_case(9, (2, inplanes, 9, 7), [spec])
    ds = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False), nn.BatchNorm2d(4 * planes)) if projection else None
    blk = M.Bottleneck(inplanes, planes, stride, ds)
    sd = blk.state_dict()
    with torch.no_grad():
        for n in sd:
            if 'num_batches' not in n:
                sd[n].copy_(params[n])
    blk = blk.to(DEV).eval()
    leaves = dict(x=leaf(x.permute(0, 2, 3, 1).contiguous()))
    leaves.update(blk.named_parameters())
    y = TO.bottleneck(leaves['x'], blk, batch_stats)
    emit(case, 'y', y)
    backward_and_emit(case, [y], [up.permute(0, 2, 3, 1)], leaves)
    for n, t in blk.state_dict().items():
        if 'running' in n:
            emit(case, n, t)


def others():
    g = torch.Generator().manual_seed(10)
    x, up = torch.randn(2, 5, 7, 32, generator=g), torch.randn(2, 10, 14, 32, generator=g)
    leaves = dict(x=leaf(x))
    y = TO.upsample2x(leaves['x'], True)
    emit('upsample2x relu', 'y', y)
    backward_and_emit('upsample2x relu', [y], [up], leaves)
    top, lat, up = (torch.randn(*s, generator=g) for s in ((2, 4, 3, 32), (2, 7, 5, 32), (2, 7, 5, 32)))
    leaves = dict(top=leaf(top), lat=leaf(lat))
    y = TO.upsample_add(leaves['top'], leaves['lat'])
    emit('upsample_add', 'y', y)
    backward_and_emit('upsample_add', [y], [up], leaves)
    x, res, up = (torch.randn(2, 5, 7, 32, generator=g) for _ in range(3))
    bn = nn.BatchNorm2d(32)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(32, generator=g))
        bn.bias.copy_(torch.randn(32, generator=g) * 0.1)
    bn.to(DEV)
    leaves = dict(x=leaf(x), res=leaf(res), gamma=bn.weight, beta=bn.bias)
    y = TO.batch_norm_act(leaves['x'], bn, True, leaves['res'], True)
    emit('batch_norm_act', 'y', y)
    backward_and_emit('batch_norm_act', [y], [up], leaves)
    emit('batch_norm_act', 'running_mean', bn.running_mean)
    emit('batch_norm_act', 'running_var', bn.running_var)


def stem_cases():
    g = torch.Generator().manual_seed(12)
    x4 = torch.nn.functional.pad(torch.randn(2, 13, 11, 3, generator=g), (0, 1)).to(DEV)
    w, up = torch.randn(32, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5, torch.randn(2, 7, 6, 32, generator=g)
    leaves = dict(w=leaf(w))
    y = TO.stem_conv(x4, leaves['w'])
    emit('stem_conv', 'y', y)
    backward_and_emit('stem_conv', [y], [up], leaves)
    x, up = torch.randn(2, 7, 6, 32, generator=g), torch.randn(2, 4, 3, 32, generator=g)
    leaves = dict(x=leaf(x))
    y = TO.max_pool_3x3_s2(leaves['x'])
    emit('max_pool_3x3_s2', 'y', y)
    backward_and_emit('max_pool_3x3_s2', [y], [up], leaves)


def wgrad_cases():
    """The two weight-gradient entries on their own: dw [K, Cout] as the kernels leave it, and db."""
    lib = L.lib()
    for k, stride, B, H, W, Cin, Cout in WGRAD_SHAPES:
        case = 'wgrad %dx%d_s%d_b%d_%dx%d_%dto%d' % (k, k, stride, B, H, W, Cin, Cout)
        g = torch.Generator().manual_seed(15)
        Ho, Wo = (down(H), down(W)) if stride == 2 else (H, W)
        x = torch.randn(B, H, W, Cin, generator=g).to(DEV)
        gy = torch.zeros(B, Ho, Wo, (Cout + 31) // 32 * 32)
        gy[..., :Cout] = torch.randn(B, Ho, Wo, Cout, generator=g)
        gy = gy.to(DEV)
        dw, db = torch.zeros(k * k * Cin, Cout, device=DEV), torch.zeros(Cout, device=DEV)
        d = L.ConvWgradDesc()
        d.x, d.g, d.dw, d.db = x.data_ptr(), gy.data_ptr(), dw.data_ptr(), db.data_ptr()
        d.B, d.H, d.W, d.Cin, d.Cout, d.ldg, d.kh, d.kw, d.pad, d.stride = B, H, W, Cin, Cout, gy.shape[3], k, k, k // 2, stride
        nbytes = lib.ymi_workspace_bytes(L.WS_CONV_WGRAD, C.byref(d))
        assert nbytes > 0, nbytes
        ws = torch.zeros(nbytes // 4, device=DEV)
        d.ws, d.ws_bytes = ws.data_ptr(), nbytes
        L.check(lib.ymi_conv_wgrad_nhwc_f32(C.byref(d), L.stream_ptr()), case)
        torch.cuda.synchronize()
        emit(case, 'dw', dw)
        emit(case, 'db', db)
    for B, H, W, Cout in STEM_WGRAD_SHAPES:
        case = 'stem_wgrad b%d_%dx%d_to%d' % (B, H, W, Cout)
        g = torch.Generator().manual_seed(16)
        x4 = torch.nn.functional.pad(torch.randn(B, H, W, 3, generator=g), (0, 1)).to(DEV)
        gy = torch.randn(B, down(H), down(W), Cout, generator=g).to(DEV)
        dw = torch.zeros(147, Cout, device=DEV)
        d = L.StemWgradDesc()
        d.x, d.g, d.dw = x4.data_ptr(), gy.data_ptr(), dw.data_ptr()
        d.B, d.H, d.W, d.Cout, d.ldg = B, H, W, Cout, Cout
        nbytes = lib.ymi_workspace_bytes(L.WS_STEM_WGRAD, C.byref(d))
        assert nbytes > 0, nbytes
        ws = torch.zeros(nbytes // 4, device=DEV)
        d.ws, d.ws_bytes = ws.data_ptr(), nbytes
        L.check(lib.ymi_stem_wgrad_nhwc_f32(C.byref(d), L.stream_ptr()), case)
        torch.cuda.synchronize()
        emit(case, 'dw', dw)


def small_net():
    """The model of test_multibox_loss_from_the_images: yolact_resnet50_config at 32 features, seeded stages, all on the GPU."""
    yolact_amd.set_cfg('yolact_resnet50_config')
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    from yolact_amd.yolact import Yolact
    torch.manual_seed(3)
    net = Yolact()
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for si, layer in enumerate(net.backbone.layers):
            for bi, blk in enumerate(layer):
                prefix = 'layers.%d.%d.' % (si, bi)
                vals = R.random_block_params(gen, blk.conv1.in_channels, blk.conv1.out_channels, blk.downsample is not None, prefix)
                for n, t in blk.state_dict().items():
                    if 'num_batches' not in n:
                        t.copy_(vals[prefix + n])
    for m in (net.backbone, net.fpn, net.proto_net, net.prediction_layers, net.semantic_seg_conv):
        m.to(DEV)
    return net, cfg


def net_case(case, net, run, inputs):
    """run(*leaves) -> dict or list of outputs; the loss is sum(output * seeded upstream gradient).  Emits every output, the gradient of
    every input and of every parameter that received one, and the running statistics; leaves the model as it found it."""
    state = {n: t.clone() for n, t in net.state_dict().items()}
    net.zero_grad(set_to_none=True)
    leaves = [leaf(t) for t in inputs]
    out = run(*leaves)
    out = out if isinstance(out, dict) else {'out%d' % i: o for i, o in enumerate(out)}
    g = torch.Generator().manual_seed(13)
    for n, o in out.items():
        emit(case, n, o)
    out = {n: o for n, o in out.items() if o.requires_grad}
    backward_and_emit(case, list(out.values()), [torch.randn(*o.shape, generator=g) for o in out.values()],
                      {'in%d' % i: t for i, t in enumerate(leaves)})
    for n, p in net.named_parameters():
        if p.grad is not None:
            emit(case, 'd_' + n, p.grad)
    for n, t in net.state_dict().items():
        if 'running' in n and not torch.equal(t, state[n]):
            emit(case, n, t)
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)


def net_cases():
    net, cfg = small_net()
    g = torch.Generator().manual_seed(14)
    images = torch.randn(2, 3, 96, 96, generator=g)
    pooled = torch.randn(2, 64, 24, 24, generator=g)
    chans = [net.backbone.channels[i] for i in cfg.backbone.selected_layers]
    convouts = [torch.randn(2, c, s, s, generator=g) for c, s in zip(chans, (12, 6, 3))]
    maps = [torch.randn(2, cfg.fpn.num_features, s, s, generator=g) for s in (12, 6, 3, 2, 1)]
    for bs in (False, True):
        mode = 'stats' if bs else 'frozen'
        net_case('forward_stem ' + mode, net, lambda: [net.forward_stem(images.to(DEV), bs)], [])
        net_case('forward_backbone ' + mode, net, lambda x: net.forward_backbone(x, bs), [pooled])
        net_case('forward_train ' + mode, net, lambda: net.forward_train(images.to(DEV), bs), [])
    net_case('forward_fpn', net, lambda *c: net.forward_fpn(list(c)), convouts)
    net_case('forward_heads', net, lambda *m: net.forward_heads(list(m)), maps)


def seed_module(mod, g):
    """Every parameter and running statistic of mod from the generator g: He-scaled filters, gamma and the running variance in
    [0.5, 1.5), small biases and means; a DCN's offset convolution small in its filters and of order one in its bias, so that the
    sampling points lie between the pixels."""
    with torch.no_grad():
        for n, t in mod.state_dict().items():
            if 'num_batches' in n:
                continue
            if 'conv_offset_mask.bias' in n:
                v = torch.randn(t.shape, generator=g)
            elif t.dim() == 4:
                v = torch.randn(t.shape, generator=g) * math.sqrt(2.0 / (t.shape[1] * t.shape[2] * t.shape[3]))
                v = v * 0.02 if 'conv_offset_mask' in n else v
            elif n.endswith('running_var') or n.endswith('weight'):
                v = 0.5 + torch.rand(t.shape, generator=g)
            else:
                v = torch.randn(t.shape, generator=g) * 0.1
            t.copy_(v)
    return mod


def emit_running(case, mod):
    for n, t in mod.state_dict().items():
        if 'running' in n:
            emit(case, n, t)


def bn_case(case, fn, shape, with_res, batch_stats, only_res=False, **kw):
    """fn = batch_norm_leaky or batch_norm_act on x of `shape`; only_res: the residual alone requires grad."""
    g = torch.Generator().manual_seed(17)
    x, res, up = (torch.randn(*shape, generator=g) for _ in range(3))
    bn = seed_module(nn.BatchNorm2d(shape[-1]), g).to(DEV).eval()
    bn.requires_grad_(not only_res)
    leaves = dict(x=leaf(x, not only_res), gamma=bn.weight, beta=bn.bias)
    if with_res:
        leaves['res'] = leaf(res)
    y = fn(leaves['x'], bn, batch_stats, leaves.get('res'), **kw)
    emit(case, 'y', y)
    backward_and_emit(case, [y], [up], leaves)
    emit_running(case, bn)


def module_case(case, fn, mod, x, batch_stats, seed):
    """fn(x, mod, batch_stats) for a seeded module on NHWC x: y, every gradient, the running statistics afterwards."""
    g = torch.Generator().manual_seed(seed)
    mod = seed_module(mod, g).to(DEV).eval()
    leaves = dict(x=leaf(torch.randn(*x, generator=g)))
    leaves.update(mod.named_parameters())
    y = fn(leaves['x'], mod, batch_stats)
    emit(case, 'y', y)
    backward_and_emit(case, [y], [torch.randn(*y.shape, generator=g)], leaves)
    emit_running(case, mod)


def deform_case(case, stride, bias):
    g = torch.Generator().manual_seed(19)
    B, H, W, Cin, Cout = 2, 6, 5, 32, 40
    Ho, Wo = (down(H), down(W)) if stride == 2 else (H, W)
    x, w, b, up = conv_inputs(g, 3, B, H, W, Cin, Cout, Ho=Ho, Wo=Wo)
    leaves = dict(x=leaf(x), om=leaf(torch.randn(B, Ho, Wo, 27, generator=g)), w=leaf(w))
    if bias:
        leaves['b'] = leaf(b)
    y = TO.deform_conv(leaves['x'], leaves['om'], leaves['w'], leaves.get('b'), stride)
    emit(case, 'y', y)
    backward_and_emit(case, [y], [up], leaves)


def darknet_net():
    """yolact_darknet53_config at 32 features around a seeded DarkNetBackbone of one block per stage."""
    yolact_amd.set_cfg('yolact_darknet53_config')
    cfg = yolact_amd.config.cfg
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    cfg.update(o)
    from yolact_amd.yolact import Yolact
    torch.manual_seed(3)
    net = Yolact()
    net.backbone = seed_module(M.DarkNetBackbone((1, 1, 1, 1, 1)), torch.Generator().manual_seed(21))
    return net.to(DEV)


def fold_cases():
    for stats in (False, True):
        mode = 'stats' if stats else 'frozen'
        for with_res in (False, True):
            bn_case('bn_leaky 2x5x7x32 %s %s' % ('res' if with_res else 'nores', mode), TO.batch_norm_leaky, (2, 5, 7, 32), with_res, stats)
        bn_case('bn_leaky 1x3x3x4 res ' + mode, TO.batch_norm_leaky, (1, 3, 3, 4), True, stats)
        bn_case('bn_leaky 2x5x7x32 only_res ' + mode, TO.batch_norm_leaky, (2, 5, 7, 32), True, stats, only_res=True)
        for relu in (True, False):
            bn_case('bn_act 2x5x7x32 only_res %s %s' % ('relu' if relu else 'norelu', mode), TO.batch_norm_act, (2, 5, 7, 32), True, stats,
                    only_res=True, relu=relu)
    g = torch.Generator().manual_seed(18)
    x4 = torch.nn.functional.pad(torch.randn(2, 9, 7, 3, generator=g), (0, 1)).to(DEV)
    w, up = torch.randn(32, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5, torch.randn(2, 9, 7, 32, generator=g)
    leaves = dict(w=leaf(w))
    y = TO.preconv(x4, leaves['w'])
    emit('preconv', 'y', y)
    backward_and_emit('preconv', [y], [up], leaves)
    for stats in (False, True):
        mode = 'stats' if stats else 'frozen'
        unit = nn.Sequential(nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(64), nn.LeakyReLU(0.1))
        module_case('dark_unit 3x3_s2_32to64 ' + mode, TO.dark_unit, unit, (2, 9, 7, 32), stats, 20)
        module_case('dark_block 64 ' + mode, TO.dark_block, M.DarkNetBlock(64, 32), (2, 5, 7, 64), stats, 20)
    for stride in (1, 2):
        for bias in (True, False):
            deform_case('deform_conv s%d %s' % (stride, 'bias' if bias else 'nobias'), stride, bias)
    for variant in ('identity', 'proj_s2'):
        inplanes, planes, stride, projection = BLOCK_SPECS[variant]
        for stats in (False, True):
            ds = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False), nn.BatchNorm2d(4 * planes)) if projection else None
            module_case('dcn_bottleneck %s %s' % (variant, 'stats' if stats else 'frozen'), TO.dcn_bottleneck,
                        M.Bottleneck(inplanes, planes, stride, ds, use_dcn=True), (2, 9, 7, inplanes), stats, 22)
    for modes in (('fp16x2', 'fp32'), ('fp32', 'fp16x2'), ('fp16x2', 'fp16x2')):
        for inside in (True, False):
            tag = 'conv_%s wgrad_%s %s' % (modes[0], modes[1], 'inside' if inside else 'behind')
            for geo in ((3, 1, 32, 128), (3, 2, 32, 128), (3, 1, 32, 40), (3, 2, 32, 40)):
                plain_case('plain 3x3_s%d_32to%d %s' % (geo[1], geo[3], tag), geo, modes, inside)
            down_case('down 3x3_32to12 ' + tag, DOWN_SHAPES[0], None, modes, inside)
            multi_case('multi 16+81+32 ' + tag, 3, modes, inside)
    net = darknet_net()
    images = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(23))
    for stats in (False, True):
        net_case('train_net.forward darknet ' + ('stats' if stats else 'frozen'), net, lambda: TN.forward(net, images.to(DEV), stats), [])


def main():
    global PER_CASE
    if sys.argv[1:] == ['--per-case']:
        PER_CASE = {}
    elif sys.argv[1:]:
        raise SystemExit('usage: train_digest.py [--per-case]')
    print('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    name = lambda s: '%dx%d_b%d_%dx%d_%dto%d' % (s[0], s[0], s[1], s[2], s[3], s[4], s[5])
    for shape in ACT_SHAPES:
        for act in ACTS:
            act_case('act %s %s' % (name(shape), act), shape, act)
    for what, grads in (('b', (False, False, True)), ('x', (True, False, False)), ('w', (False, True, False))):
        act_case('act %s relu only_%s' % (name(ACT_SHAPES[0]), what), ACT_SHAPES[0], 'relu', grads)
    act_case('act %s tanh float64' % name(ACT_SHAPES[0]), ACT_SHAPES[0], 'tanh', dtype=torch.float64)
    multi_case('multi 16+81+32 all', 3)
    multi_case('multi 16+81+32 first_two', 2)
    for shape in DOWN_SHAPES:
        for act in ACTS:
            down_case('down %s %s' % (name(shape), act), shape, act)
    for geo in PLAIN_GEOS:
        plain_case('plain %dx%d_s%d_%dto%d' % (geo[0], geo[0], geo[1], geo[2], geo[3]), geo)
    for variant, spec in BLOCK_SPECS.items():
        for batch_stats in (False, True):
            block_case('bottleneck %s %s' % (variant, 'stats' if batch_stats else 'frozen'), spec, batch_stats)
    others()
    stem_cases()
    wgrad_cases()
    net_cases()
    fold_cases()
    for case, lines in (PER_CASE or {}).items():
        # the SHA-256 of the case's lines as the plain run prints them, each ended by a newline
        print('%-62s %4d %s' % (case, len(lines), hashlib.sha256(''.join(l + '\n' for l in lines).encode()).hexdigest()))


if __name__ == '__main__':
    main()
