"""Generate tests/golden/mask_loss.npz by EXECUTING THE REFERENCE's MultiBoxLoss.lincomb_mask_loss on the CPU (build container only).

    python tools/make_golden_mask_loss.py            # needs the reference checkout; writes tests/golden/mask_loss.npz

The reference is imported with the stubs of oracle/make_golden._shim_reference under yolact_base_config, whose
mask-loss switches are those of every shipped base config.  Per case the file holds the method's inputs (pos, idx_t, mask_data,
proto_data, the image-size GT masks, gt_box_t), its result 'M', d M / d proto_data, d M / d mask_data, and — for the case over
cfg.masks_to_train — the `select` it drew from torch.randperm after torch.manual_seed(meta torch_seed).  Only data is stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

#        name        mh  mw  positives per image   priors  seed
CASES = [('tile12x10', 12, 10, (3,), 8, 11),
         ('ragged17x19', 17, 19, (5, 0, 20), 32, 12),
         ('overcap12x10', 12, 10, (130,), 140, 13)]
TORCH_SEED = 1234
UP = 2                                                # GT masks are UP x the prototype size


def make_inputs(mh, mw, ns, P, seed):
    """Seeded inputs of lincomb_mask_loss: GT = ellipses inscribed in random boxes, gt_box_t = the box of the matched GT."""
    g = torch.Generator().manual_seed(seed)
    B, H, W = len(ns), mh * UP, mw * UP
    proto = torch.relu(torch.randn(B, mh, mw, 32, generator=g)) * 0.5
    mask_data = torch.tanh(torch.randn(B, P, 32, generator=g))
    pos = torch.zeros(B, P, dtype=torch.bool)
    idx_t = torch.zeros(B, P, dtype=torch.long)
    gt_box_t = torch.zeros(B, P, 4)
    masks, labels = [], []
    yy = (torch.arange(H).float() + 0.5).view(H, 1) / H
    xx = (torch.arange(W).float() + 0.5).view(1, W) / W
    for b in range(B):
        n_gt = 3 + b
        c = 0.2 + 0.6 * torch.rand(n_gt, 2, generator=g)
        half = 0.08 + 0.25 * torch.rand(n_gt, 2, generator=g)
        box = torch.cat([c - half, c + half], 1).clamp(0.01, 0.99)                  # x1, y1, x2, y2
        cx, cy = (box[:, 0] + box[:, 2]) / 2, (box[:, 1] + box[:, 3]) / 2
        rx, ry = (box[:, 2] - box[:, 0]) / 2, (box[:, 3] - box[:, 1]) / 2
        m = (((xx.unsqueeze(0) - cx.view(-1, 1, 1)) / rx.view(-1, 1, 1)) ** 2
             + ((yy.unsqueeze(0) - cy.view(-1, 1, 1)) / ry.view(-1, 1, 1)) ** 2) <= 1.0
        masks.append(m.float())
        labels.append(torch.randint(1, 81, (n_gt,), generator=g))
        chosen = torch.randperm(P, generator=g)[:ns[b]]
        pos[b, chosen] = True
        idx_t[b] = torch.randint(0, n_gt, (P,), generator=g)
        gt_box_t[b] = box[idx_t[b]]
    return proto, mask_data, pos, idx_t, gt_box_t, masks, labels


def run_reference(crit, inputs):
    proto, mask_data, pos, idx_t, gt_box_t, masks, labels = inputs
    proto = proto.clone().requires_grad_(True)
    mask_data = mask_data.clone().requires_grad_(True)
    drawn = []
    real = torch.randperm

    def randperm(*a, **k):
        perm = real(*a, **k)
        drawn.append(perm.clone())
        return perm
    torch.manual_seed(TORCH_SEED)
    torch.randperm = randperm
    try:
        losses = crit.lincomb_mask_loss(pos, idx_t, None, mask_data, None, proto, masks, gt_box_t, None, None, labels)
    finally:
        torch.randperm = real
    M = losses['M']
    dp, dm = torch.autograd.grad(M, [proto, mask_data])
    return M.detach(), dp, dm, drawn


def main():
    from oracle.make_golden import _shim_reference
    _shim_reference()
    from data import cfg, set_cfg
    set_cfg('yolact_base_config')
    from layers.modules.multibox_loss import MultiBoxLoss
    assert cfg.mask_proto_crop and cfg.mask_proto_normalize_emulate_roi_pooling and cfg.mask_proto_binarize_downsampled_gt
    assert cfg.masks_to_train == 100 and cfg.mask_alpha == 6.125 and not cfg.use_maskiou
    crit = MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3)
    arrays, metas = {}, []
    for name, mh, mw, ns, P, seed in CASES:
        inputs = make_inputs(mh, mw, ns, P, seed)
        M, dp, dm, drawn = run_reference(crit, inputs)
        proto, mask_data, pos, idx_t, gt_box_t, masks, _ = inputs
        arrays.update({name + '_proto': proto.numpy(), name + '_mask_data': mask_data.numpy(), name + '_pos': pos.numpy(),
                       name + '_idx_t': idx_t.numpy(), name + '_gt_box_t': gt_box_t.numpy(),
                       name + '_M': M.numpy().astype(np.float32), name + '_d_proto': dp.numpy(), name + '_d_mask_data': dm.numpy()})
        for b, m in enumerate(masks):
            arrays['%s_masks_%d' % (name, b)] = m.numpy().astype(np.uint8)
        over = [b for b, n in enumerate(ns) if n > cfg.masks_to_train]
        assert len(over) == len(drawn)
        for b, perm in zip(over, drawn):
            arrays['%s_select_%d' % (name, b)] = perm[:cfg.masks_to_train].numpy().astype(np.int64)
        metas.append(dict(name=name, mh=mh, mw=mw, ns=list(ns), P=P, seed=seed, over_cap=over))
        print('%-14s M = %.6f  |d_proto| max %.3e  |d_mask_data| max %.3e  draws %d'
              % (name, float(M), dp.abs().max().item(), dm.abs().max().item(), len(drawn)))
    meta = dict(cases=metas, torch_seed=TORCH_SEED, masks_to_train=int(cfg.masks_to_train), mask_alpha=float(cfg.mask_alpha),
                torch=torch.__version__)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'mask_loss.npz')
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
