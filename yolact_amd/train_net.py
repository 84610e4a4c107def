"""The train-mode network: the reference's TRAIN-mode Yolact.forward (yolact.py:564-647) as plain functions on NHWC fp32 GPU tensors,
each a sequence of layers/train_ops.py calls (the HIP kernels) and once differentiable like them.  `net` is a Yolact; its plans are not
touched.  stem (which takes the NCHW image: it builds x4 itself) -> backbone -> fpn (of the selected stages) -> heads; forward is their
composition.  A DarkNetBackbone (yolact_darknet53) goes through darknet in place of stem -> backbone.  Nothing here validates:
Yolact.forward_stem / .. / forward_train check the model, cfg and the tensors and change the layout.  What shows only layer by layer (a make_net or downsample layer the kernels do not take) raises here, named after the Yolact
method.  The ORDER of the train_ops calls is part of the contract: autograd adds the gradients of a map's consumers in node order.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import modules as M
from .config import act_name, make_priors_host
from .layers import train_ops as TO


def conv_of(x, m, act, w=None, b=None):
    """TO.conv2d_act with the geometry of the nn.Conv2d m, on its own parameters or on the aliases (w, b) of them."""
    return TO.conv2d_act(x, m.weight if w is None else w, m.bias if b is None else b, m.padding, act, stride=m.stride,
                         dilation=m.dilation, groups=m.groups)


def image4(x_nchw):
    """The NCHW image as NHWC fp32 with a fourth channel of zeros, built once with torch operations and detached: what stem_conv and
    preconv read, forward and backward."""
    return nn.functional.pad(x_nchw.detach().to(torch.float32).permute(0, 2, 3, 1), (0, 1)).contiguous()


def apply_net(seq, x, last_act=None, params=None):
    """A make_net Sequential (utils/functions.py:163-213) on NHWC x through layers/train_ops: Conv2d (+ the ReLU behind it),
    InterpolateModule (+ the ReLU behind it).  last_act: the activation applied after a final layer that has no ReLU of its own.
    params: [w, b, w, b, ..] to use in place of the convolutions' own parameters (aliases of a shared head)."""
    mods = list(seq)
    params = None if params is None else list(params)
    for i, m in enumerate(mods):
        if isinstance(m, nn.ReLU):
            continue
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        act = 'relu' if relu else (last_act if i == len(mods) - 1 else None)
        if isinstance(m, nn.Conv2d):
            x = conv_of(x, m, act) if params is None else conv_of(x, m, act, params.pop(0), params.pop(0))
        elif isinstance(m, M.InterpolateModule):
            if m.scale_factor != 2 or act not in (None, 'relu'):
                raise NotImplementedError('yolact_amd forward_heads: an interpolation by %r followed by %r is not supported '
                                          '(x2 bilinear with or without ReLU is)' % (m.scale_factor, act))
            x = TO.upsample2x(x, relu=act == 'relu')
        else:
            raise NotImplementedError('yolact_amd forward_heads: layer %r is not implemented' % (m,))
    return x


def priors(net, sizes, cfg, device):
    """The priors of heads(): built on the host once per (level sizes, every cfg value they are made from, device) and kept on the
    device, as the reference keeps them per map size (yolact.py:214-263); cfg is still read at every call.  The cache is net's."""
    bbc = cfg.backbone
    nlev = len(sizes)
    freeze = lambda v: tuple(freeze(e) for e in v) if isinstance(v, (list, tuple)) else v
    key = (tuple(sizes), freeze(list(bbc.pred_scales[:nlev])), freeze(list(bbc.pred_aspect_ratios[:nlev])), cfg.max_size,
           bool(bbc.use_pixel_scales), bool(bbc.preapply_sqrt), bool(bbc.use_square_anchors), str(device))
    cache = net.__dict__.setdefault('_train_prior_cache', {})
    pri = cache.get(key)
    if pri is None:
        data = []
        for lvl, (h, w) in enumerate(sizes):
            data += make_priors_host(h, w, bbc.pred_scales[lvl], bbc.pred_aspect_ratios[lvl], cfg.max_size, bbc)
        if len(cache) >= 8:
            cache.clear()
        pri = cache[key] = torch.tensor(data, dtype=torch.float32).view(-1, 4).to(device)
    return pri


def stem(net, x_nchw, batch_stats=None):
    """conv1, bn1, ReLU, max-pool (backbone.py:129-132).  The image is padded to NHWC with a fourth channel of zeros once, with torch
    operations; the convolution's backward reads that same tensor."""
    bb = net.backbone
    with torch.cuda.device(x_nchw.device):
        y = TO.stem_conv(image4(x_nchw), bb.conv1.weight)
        y = TO.batch_norm_act(y, bb.bn1, batch_stats, relu=True)
        return TO.max_pool_3x3_s2(y)


def backbone(net, x, batch_stats=None):
    """The ResNet stages behind the stem (backbone.py:135-142) -> one output per stage.  A DCN block (use_dcn = True, the YOLACT++
    configs) runs through TO.dcn_bottleneck: the Yolact methods still refuse such a model in _check_backbone, so only a caller of
    this module reaches it."""
    outs = []
    with torch.cuda.device(x.device):
        for layer in net.backbone.layers:
            for block in layer:
                x = (TO.dcn_bottleneck if getattr(block, 'use_dcn', False) else TO.bottleneck)(x, block, batch_stats)
            # an alias made HERE, before the next stage exists: autograd runs its node after the next stage's, so what comes back
            # through a stage's output (the FPN's lateral) is added to that map's gradient last, with or without a layout change
            # between the stages.  forward() and the chain of Yolact's four methods then give the same gradient bits.
            outs.append(x.view_as(x))
    return outs


def darknet(net, x_nchw, batch_stats=None):
    """A DarkNetBackbone (backbone.py:252-294) on the NCHW image -> one output per stage: the image padded to NHWC-4 as in stem, the
    _preconv unit, then five stages, each a stride-2 unit followed by its DarkNetBlocks.  Yolact's methods refuse a DarkNet, so only
    a caller of this module (forward, below) reaches it; check_darknet names what the kernels do not take."""
    bb = net.backbone
    TO.check_darknet(bb)
    outs = []
    with torch.cuda.device(x_nchw.device):
        conv, bn = bb._preconv[0], bb._preconv[1]
        x = TO.batch_norm_leaky(TO.preconv(image4(x_nchw), conv.weight), bn, batch_stats)
        for layer in bb.layers:
            mods = list(layer)
            x = TO.dark_unit(x, mods[0], batch_stats)
            for block in mods[1:]:
                x = TO.dark_block(x, block, batch_stats)
            # the alias backbone() makes, for its reason: a stage output has two consumers (the next stage and the FPN's lateral)
            outs.append(x.view_as(x))
    return outs


def fpn(net, feats):
    """FPN.forward (yolact.py:311-360) on the selected stage outputs, finest first, for the variant Yolact.__init__ insists on."""
    f = net.fpn
    n = len(feats)
    with torch.cuda.device(feats[0].device):
        # lat_layers and pred_layers are stored deepest level first (yolact.py:286-296, 324-341)
        out, x = [None] * n, None
        for i, lat in enumerate(f.lat_layers):
            j = n - 1 - i
            lateral = conv_of(feats[j], lat, None)
            x = lateral if x is None else TO.upsample_add(x, lateral)
            out[j] = x
        for i, pred in enumerate(f.pred_layers):
            j = n - 1 - i
            out[j] = conv_of(out[j], pred, 'relu')
        for down in f.downsample_layers:
            if tuple(down.stride) != (2, 2) or tuple(down.padding) != (down.kernel_size[0] // 2,) * 2 or \
                    tuple(down.dilation) != (1, 1) or down.groups != 1:
                raise NotImplementedError('yolact_amd forward_fpn: downsample layer %r is not supported (stride 2, padding k // 2 is)'
                                          % (down,))
            out.append(TO.conv2d_down(out[-1], down.weight, down.bias))
    return out


def heads(net, feats):
    """The pyramid maps -> pred_outs (yolact.py:579-647), the dict Yolact.forward_heads describes."""
    cfg = net.cfg
    B = feats[0].shape[0]
    pm = net.prediction_layers[0]
    coef_act = act_name(cfg.mask_proto_coeff_activation)
    proto_act = act_name(cfg.mask_proto_prototype_activation)
    with torch.cuda.device(feats[0].device):
        proto = apply_net(net.proto_net, feats[net.proto_src], last_act=None if proto_act == 'none' else proto_act)
        loc, conf, mask = [], [], []
        up = [m for m in pm.upfeature if isinstance(m, nn.Conv2d)] if hasattr(pm, 'upfeature') else []
        hl = pm.bbox_layer
        # one set of weights on every level: each level works on aliases whose gradients are added in level order
        shared = TO.share_params(len(feats), [t for m in up + [pm.bbox_layer, pm.conf_layer, pm.mask_layer]
                                              for t in (m.weight, m.bias)])
        for lvl, x in enumerate(feats):
            hp = shared[lvl]
            if up:
                x = apply_net(pm.upfeature, x, params=hp[:2 * len(up)])
            wb, bb_, wc, bc, wm, bm = hp[2 * len(up):]
            b, c, m = TO.conv2d_multi(x, [(wb, bb_, None), (wc, bc, None), (wm, bm, coef_act)],
                                      hl.padding, stride=hl.stride, dilation=hl.dilation, groups=hl.groups)
            loc.append(b.reshape(B, -1, 4))
            conf.append(c.reshape(B, -1, cfg.num_classes))
            mask.append(m.reshape(B, -1, net.mask_dim))
        pred = {'loc': torch.cat(loc, 1), 'conf': torch.cat(conf, 1), 'mask': torch.cat(mask, 1),
                'priors': priors(net, [tuple(f.shape[1:3]) for f in feats], cfg, feats[0].device), 'proto': proto}
        if cfg.use_semantic_segmentation_loss:
            pred['segm'] = conv_of(feats[0], net.semantic_seg_conv, None).permute(0, 3, 1, 2)
    return pred


def forward(net, x_nchw, batch_stats=None):
    """The image batch [B,3,H,W] -> pred_outs, without a layout change between the stages.  Writes cfg._tmp_img_h / _w (the image
    size the criterion reads, yolact.py:566-567) as Yolact.forward_train does, so a caller that comes here directly needs no method
    of Yolact."""
    net.cfg._tmp_img_h, net.cfg._tmp_img_w = int(x_nchw.shape[2]), int(x_nchw.shape[3])
    if isinstance(net.backbone, M.DarkNetBackbone):
        outs = darknet(net, x_nchw, batch_stats)
    else:
        outs = backbone(net, stem(net, x_nchw, batch_stats), batch_stats)
    return heads(net, fpn(net, [outs[i] for i in net.cfg.backbone.selected_layers]))
