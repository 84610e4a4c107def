"""Generate tests/golden/maskiou.npz by EXECUTING THE REFERENCE's lincomb_mask_loss and mask_iou_loss on the CPU (build container only).

    python tools/make_golden_maskiou.py              # needs the reference checkout; writes tests/golden/maskiou.npz

The reference is imported with the stubs of oracle/make_golden._shim_reference under yolact_plus_base_config (use_maskiou,
maskiou_alpha 25, discard_mask_area 25).  To keep the fixture small the prototypes are 24 x 24 for two images and cfg.maskiou_net is
three layers, [(8,3,s2), (16,3,s2), (32,3,s2)] plus the 1x1 convolution to 80: the maps go 24 -> 11 -> 5 -> 2, the pool has four
candidates.  The net is the reference's own FastMaskIoUNet with seeded parameters.

The case, on the 114 priors of the multibox golden: image 0 has three objects and a crowd - one box touches the left border, one
is so small that its downsampled GT covers <= 25 pixels and the reference discards it - image 1 has two objects.  pos, idx_t and
gt_box_t come from tests/match_ref.py (pinned to the reference's match by tests/golden/match.npz).  Stored: the inputs (mask
coefficients multiples of 1/1024, prototypes of 1/256, as fp16, which holds them exactly: every logit is then exact in fp32), the
net's parameters, 'M', 'I', maskiou_t, label_t, the selection (the rows of an all-instances run that the discarding run kept) and the
gradients of M + I in mask, proto and the net's eight parameters.  Only data is stored.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PYRAMID, MAX_SIZE, MH, NET = (5, 3, 2), 138, 24, [(8, 3, {'stride': 2}), (16, 3, {'stride': 2}), (32, 3, {'stride': 2})]
GEO = ((3, 3, 2, 0, 1),) * 3 + ((1, 1, 1, 0, 1),)


def main():
    from oracle.make_golden import _shim_reference
    _shim_reference()
    from data import cfg, set_cfg
    set_cfg('yolact_plus_base_config')
    cfg.maskiou_net = NET
    import layers.modules.multibox_loss as mod
    import yolact as ref_yolact
    import maskiou_loss_ref as IR
    from make_golden_multibox import grid
    from match_ref import make_priors, match_batch_ref
    assert cfg.use_maskiou and cfg.maskiou_alpha == 25 and cfg.discard_mask_area == 25 and cfg.maskious_to_train == -1
    assert cfg.mask_proto_crop and cfg.mask_proto_normalize_emulate_roi_pooling and cfg.masks_to_train == 100
    crit = mod.MultiBoxLoss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)
    priors = make_priors(PYRAMID, MAX_SIZE)
    P = priors.size(0)
    g = torch.Generator().manual_seed(57)

    row = lambda box, cls: box + [float(cls)]
    targets = [torch.tensor([row([0.0, 0.2, 0.45, 0.7], 3), row([0.5, 0.5, 0.95, 0.9], 17), row([0.6, 0.1, 0.75, 0.25], 60),
                             row([0.3, 0.3, 0.8, 0.8], -1)]),
               torch.tensor([row([0.1, 0.1, 0.6, 0.55], 40), row([0.55, 0.4, 1.0, 1.0], 3)])]
    targets = [torch.cat([grid(t[:, :4], 1024), t[:, 4:]], 1) for t in targets]
    num_crowds = [1, 0]
    masks = []
    for t in targets:                                                   # a 48 x 48 mask per annotation: its box, with a hole
        m = torch.zeros(t.size(0), 48, 48)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 48).round().long().tolist()):
            m[j, y1:y2, x1:x2] = 1
            m[j, (y1 + y2) // 2, (x1 + x2) // 2] = 0
        masks.append(m)
    mt = match_batch_ref(priors, targets, num_crowds)
    pos, idx_t, gt_box_t = mt['pos'], mt['idx_t'], mt['gt_box_t']
    obj_masks = [m[:m.size(0) - nc] for m, nc in zip(masks, num_crowds)]
    labels = [t[:t.size(0) - nc, 4].long() for t, nc in zip(targets, num_crowds)]
    mask = grid(torch.tanh(torch.randn(2, P, 32, generator=g)), 1024)
    proto = grid(torch.relu(torch.randn(2, MH, MH, 32, generator=g)) * 0.5, 256)
    params = IR.make_params(g, (8, 16, 32, 80), GEO)

    net = types.SimpleNamespace(maskiou_net=ref_yolact.FastMaskIoUNet())
    convs = [m for m in net.maskiou_net.maskiou_net if isinstance(m, torch.nn.Conv2d)]
    assert [tuple(c.weight.shape) for c in convs] == [tuple(p.shape) for p in params[0::2]]
    with torch.no_grad():
        for c, w, b in zip(convs, params[0::2], params[1::2]):
            c.weight.copy_(w)
            c.bias.copy_(b)
    leaves_net = [t for c in convs for t in (c.weight, c.bias)]

    def run(discard):
        cfg.discard_mask_area = discard
        lm, lp = mask.clone().requires_grad_(True), proto.clone().requires_grad_(True)
        state = torch.random.get_rng_state()
        losses, tg = crit.lincomb_mask_loss(pos, idx_t, None, lm, priors, lp, [m.clone() for m in obj_masks], gt_box_t, None, None,
                                            labels)
        assert torch.equal(state, torch.random.get_rng_state())        # no randperm was drawn
        return losses, tg, lm, lp

    _, tg_all, _, _ = run(-1)
    losses, tg, lm, lp = run(25)
    cfg.discard_mask_area = 25
    I = crit.mask_iou_loss(net, tg)
    grads = torch.autograd.grad(losses['M'] + I, [lm, lp] + leaves_net)
    # the selection: the rows of the all-instances run that the discarding run kept, in order
    n_all, n = tg_all[0].size(0), tg[0].size(0)
    select, at = torch.zeros(n_all, dtype=torch.bool), 0
    for j in range(n_all):
        if at < n and torch.equal(tg_all[0][j], tg[0][at]) and tg_all[2][j] == tg[2][at]:
            select[j] = True
            at += 1
    assert at == n and 0 < n < n_all
    assert torch.equal(tg_all[1][select], tg[1])
    boxes = torch.cat([gt_box_t[b, pos[b]] for b in range(2)])
    assert (boxes[select][:, 0] == 0).any()                            # a kept instance touches the border
    print('positives %s, %d instances, %d kept; M = %.6f  I = %.6f  maskiou_t %s' % (pos.sum(1).tolist(), n_all, n, float(losses['M']), float(I),
                                                                                       ['%.4f' % v for v in tg[1].tolist()]))

    f16 = lambda t: t.numpy().astype(np.float16)
    arrays = dict(priors=priors.numpy(), mask=f16(mask), proto=f16(proto), M=losses['M'].detach().numpy().reshape(1),
                  I=I.detach().numpy().reshape(1), maskiou_t=tg[1].numpy(), maskiou_t_all=tg_all[1].numpy(), label_t=tg[2].numpy().astype(np.int16),
                  select=select.numpy().astype(np.uint8), d_mask=grads[0].numpy(), d_proto=grads[1].numpy())
    for b in range(2):
        arrays['targets_%d' % b] = targets[b].numpy()
        arrays['masks_%d' % b] = masks[b].numpy().astype(np.uint8)
    for i, (p, d) in enumerate(zip(params, grads[2:])):
        arrays['param_%d' % i] = p.numpy()
        arrays['d_param_%d' % i] = d.numpy()
    meta = dict(P=P, pyramid=list(PYRAMID), max_size=MAX_SIZE, num_crowds=num_crowds, geo=[list(x) for x in GEO], maskiou_alpha=25.0,
                discard_mask_area=25, mask_alpha=6.125, n_params=len(params), torch=torch.__version__)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'maskiou.npz')
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < 320 * 1024


if __name__ == '__main__':
    main()
