"""Generate tests/golden/multibox.npz by EXECUTING THE REFERENCE's MultiBoxLoss on the CPU (build container only).

    python tools/make_golden_multibox.py             # needs the reference checkout; writes tests/golden/multibox.npz

The reference is imported with the stubs of oracle/make_golden._shim_reference under yolact_base_config.  Three things are
recorded, on 114 priors (pyramid 5, 3, 2), 81 classes:

    ohem_*   MultiBoxLoss.ohem_conf_loss called directly: `ohemA` (two images: one with neutrals, one WITHOUT positives) and
             `ohemB` (one image whose 3 * num_pos is clamped to P - 1).  conf_t is made by hand.  Stored: conf, conf_t, 'C', d C / d
             conf, neg (the non-positive rows the reference's gradient touches) and n (the reference's own clamped num_neg, read
             off its torch.clamp call).
    segm_*   MultiBoxLoss.semantic_segmentation_loss called directly on the forward case's segm, masks and labels: 'S', d S / d segm.
    segm2_*  the same on a 2 x 80 x 5 x 4 map where two OVERLAPPING objects of image 0 share a class (the OR of :235).
    fwd_*    one full forward() with crowds and fewer than masks_to_train positives per image (no randperm is drawn): the inputs,
             the four normalised losses and the gradients of their sum in loc, conf, mask, proto and segm.

Logits stay within +-8 (the reference's log_sum_exp subtracts the batch maximum; at this range its key is well conditioned) and
every image's cut - the last selected against the first unselected key - is opened to at least 1e-3 by raising row[0] of the first
unselected row (tests/class_loss_ref.open_the_cuts), asserted here on the reference's own keys.  Inputs are multiples of 1/64 (1/256,
1/1024) and stored as fp16, which holds them exactly; only data is stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PYRAMID, MAX_SIZE, NUM_CLASSES, GAP = (5, 3, 2), 138, 81, 1e-3


def grid(t, step):
    """t rounded to multiples of 1 / step: exact in fp16 for |t| < 2048 / step."""
    q = torch.round(t * step) / step
    assert torch.equal(q.half().float(), q)
    return q


def logits(g, *shape):
    return grid((torch.randn(*shape, generator=g) * 2.0).clamp(-8, 8), 64)


def reference_keys(conf, conf_t):
    """The reference's own mining keys (multibox_loss.py:244-256), for the gap assertion."""
    from layers.box_utils import log_sum_exp
    flat = conf.view(-1, conf.size(2))
    k = (log_sum_exp(flat) - flat[:, 0]).view(conf.size(0), -1).clone()
    k[conf_t != 0] = 0
    return k


def assert_gaps(conf, conf_t, ratio):
    from class_loss_ref import cut_gaps
    pos = conf_t > 0
    n = (ratio * pos.sum(1)).clamp(max=conf.size(1) - 1)
    gaps = cut_gaps(reference_keys(conf, conf_t), n)
    assert min(gaps) >= GAP, gaps
    return gaps


def run_ohem(crit, conf, conf_t):
    """-> ('C', d_conf, neg, n) of the reference's ohem_conf_loss."""
    seen = []
    real = torch.clamp

    def clamp(*a, **k):
        out = real(*a, **k)
        seen.append(out)
        return out
    x = conf.clone().requires_grad_(True)
    pos = conf_t > 0
    torch.clamp = clamp
    try:
        loss = crit.ohem_conf_loss(x, conf_t, pos, conf.size(0))
    finally:
        torch.clamp = real
    (d,) = torch.autograd.grad(loss, [x])
    assert len(seen) == 1                                               # :260
    neg = (d != 0).any(2) & ~pos
    return loss.detach(), d, neg, seen[0].view(-1)


def main():
    from oracle.make_golden import _shim_reference
    _shim_reference()
    from data import cfg, set_cfg
    set_cfg('yolact_base_config')
    import layers.modules.multibox_loss as mod
    from class_loss_ref import open_the_cuts
    from make_golden_match import random_targets
    from match_ref import make_priors, match_batch_ref
    assert not cfg.use_focal_loss and not cfg.use_objectness_score and not cfg.ohem_use_most_confident and not cfg.use_class_balanced_conf
    assert cfg.use_semantic_segmentation_loss and cfg.mask_proto_loss is None and not cfg.use_maskiou and cfg.train_masks
    assert (cfg.conf_alpha, cfg.semantic_segmentation_alpha, cfg.ohem_negpos_ratio, cfg.num_classes) == (1, 1, 3, NUM_CLASSES)
    crit = mod.MultiBoxLoss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)
    priors = make_priors(PYRAMID, MAX_SIZE)
    P = priors.size(0)
    assert P == 114
    g = torch.Generator().manual_seed(41)
    arrays = {}
    f16 = lambda t: t.numpy().astype(np.float16)

    # ---- the forward case: image 0 with 3 objects + 1 crowd, image 1 with 2 objects -------------------------------------------
    num_crowds = [1, 0]
    targets = [random_targets(g, 3, 1), random_targets(g, 2, 0)]
    targets = [torch.cat([grid(t[:, :4], 1024), t[:, 4:]], 1) for t in targets]
    masks = []
    for t in targets:                                                   # a 32x32 mask per annotation: its box, with a hole
        m = torch.zeros(t.size(0), 32, 32)
        for j, (x1, y1, x2, y2) in enumerate((t[:, :4] * 32).round().long().tolist()):
            m[j, y1:max(y2, y1 + 2), x1:max(x2, x1 + 2)] = 1
            m[j, (y1 + y2) // 2, (x1 + x2) // 2] = 0
        masks.append(m)
    ref_match = match_batch_ref(priors, targets, num_crowds)
    conf_t_fwd = ref_match['conf_t']
    assert (conf_t_fwd < 0).any() and (conf_t_fwd > 0).sum(1).min() >= 1 and (conf_t_fwd > 0).sum(1).max() < cfg.masks_to_train
    conf = open_the_cuts(logits(g, 2, P, NUM_CLASSES), conf_t_fwd, 3, 4 * GAP)
    grid(conf, 64)
    loc = grid(torch.randn(2, P, 4, generator=g) * 0.7, 256)
    mask = grid(torch.tanh(torch.randn(2, P, 32, generator=g)), 1024)
    proto = grid(torch.relu(torch.randn(2, 12, 12, 32, generator=g)) * 0.5, 256)
    segm = logits(g, 2, NUM_CLASSES - 1, 8, 8)
    leaves = [t.clone().requires_grad_(True) for t in (loc, conf, mask, proto, segm)]
    preds = dict(loc=leaves[0], conf=leaves[1], mask=leaves[2], priors=priors, proto=leaves[3], segm=leaves[4])
    seen = {}
    real_ohem = crit.ohem_conf_loss

    def ohem(conf_data, conf_t, pos, num):
        seen['conf_t'] = conf_t.clone()
        return real_ohem(conf_data, conf_t, pos, num)
    crit.ohem_conf_loss = ohem
    torch.manual_seed(7)
    state = torch.random.get_rng_state()
    losses = crit(None, preds, [t.clone() for t in targets], [m.clone() for m in masks], list(num_crowds))
    assert torch.equal(state, torch.random.get_rng_state())            # no randperm was drawn
    crit.ohem_conf_loss = real_ohem
    assert sorted(losses) == ['B', 'C', 'M', 'S']
    assert torch.equal(seen['conf_t'], conf_t_fwd)
    assert_gaps(conf, conf_t_fwd, 3)
    grads = torch.autograd.grad(sum(losses.values()), leaves)
    arrays.update(priors=priors.numpy(), fwd_loc=f16(loc), fwd_conf=f16(conf), fwd_mask=f16(mask), fwd_proto=f16(proto),
                  fwd_segm=f16(segm), fwd_conf_t=conf_t_fwd.numpy().astype(np.int16))
    for b in range(2):
        arrays['fwd_targets_%d' % b] = targets[b].numpy()
        arrays['fwd_masks_%d' % b] = masks[b].numpy().astype(np.uint8)
    for k, v in losses.items():
        arrays['fwd_' + k] = v.detach().numpy().astype(np.float32).reshape(1)
    for name, d in zip(('loc', 'conf', 'mask', 'proto', 'segm'), grads):
        arrays['fwd_d_' + name] = d.numpy()
    print('forward: positives %s neutrals %s  %s' % ((conf_t_fwd > 0).sum(1).tolist(), (conf_t_fwd < 0).sum(1).tolist(),
                                                      {k: v.item() for k, v in losses.items()}))

    # ---- semantic_segmentation_loss directly, on the forward case's segm and its non-crowd masks and labels --------------------
    obj_masks = [m[:m.size(0) - nc] for m, nc in zip(masks, num_crowds)]
    labels = [t[:t.size(0) - nc, 4].long() for t, nc in zip(targets, num_crowds)]
    x = segm.clone().requires_grad_(True)
    S = crit.semantic_segmentation_loss(x, obj_masks, labels)
    (dS,) = torch.autograd.grad(S, [x])
    arrays.update(segm_S=S.detach().numpy().astype(np.float32).reshape(1), segm_d_segm=dS.numpy())

    # ---- ohem_conf_loss directly ----------------------------------------------------------------------------------------------
    # ohemA: the forward case's logits; image 0 with 9 positives and 12 neutrals, image 1 without positives
    ct = torch.zeros(2, P, dtype=torch.long)
    perm = torch.randperm(P, generator=g)
    ct[0, perm[:9]] = torch.randint(1, NUM_CLASSES, (9,), generator=g)
    ct[0, perm[9:21]] = -1
    ct[1, perm[:6]] = -1
    # ohemB: 40 positives of 114: 3 * 40 is clamped to 113, every negative is mined
    ctb = torch.zeros(1, P, dtype=torch.long)
    ctb[0, torch.randperm(P, generator=g)[:40]] = torch.randint(1, NUM_CLASSES, (40,), generator=g)
    confb = logits(g, 1, P, NUM_CLASSES)
    for name, c, t in (('ohemA', open_the_cuts(conf, ct, 3, 4 * GAP), ct), ('ohemB', open_the_cuts(confb, ctb, 3, 4 * GAP), ctb)):
        grid(c, 64)
        gaps = assert_gaps(c, t, 3)
        C, d, neg, n = run_ohem(crit, c, t)
        arrays.update({name + '_conf': f16(c), name + '_conf_t': t.numpy().astype(np.int16),
                       name + '_C': C.numpy().astype(np.float32).reshape(1), name + '_d_conf': d.numpy(),
                       name + '_neg': neg.numpy().astype(np.uint8), name + '_n': n.numpy().astype(np.int32)})
        print('%s: positives %s neutrals %s n %s negatives %s gaps %s C = %.6f'
              % (name, (t > 0).sum(1).tolist(), (t < 0).sum(1).tolist(), n.tolist(), neg.sum(1).tolist(),
                 ['%.2e' % v for v in gaps], float(C)))
    assert arrays['ohemA_n'].tolist() == [27, 0] and arrays['ohemB_n'].tolist() == [P - 1]
    assert arrays['ohemB_neg'].sum() == P - 40

    # ---- semantic_segmentation_loss directly, two OVERLAPPING objects of one class in image 0 (the OR of :235) -----------------
    # 20x16 masks in blocks of 4, so that the 5x4 downsample is exact: A covers rows 0-2 / cols 0-1, B rows 2-4 / cols 1-3 of the
    # small map, they share the pixel (2, 1) and each has pixels of its own; a third object of another class; image 1 has one object
    m0 = torch.zeros(3, 20, 16)
    m0[0, 0:12, 0:8] = 1
    m0[1, 8:20, 4:16] = 1
    m0[2, 4:16, 8:16] = 1
    m1 = torch.zeros(1, 20, 16)
    m1[0, 0:8, 0:16] = 1
    masks2, labels2 = [m0, m1], [torch.tensor([19, 19, 54]), torch.tensor([7])]
    segm2 = logits(g, 2, NUM_CLASSES - 1, 5, 4)
    x = segm2.clone().requires_grad_(True)
    S2 = crit.semantic_segmentation_loss(x, masks2, labels2)
    (dS2,) = torch.autograd.grad(S2, [x])
    arrays.update(segm2_segm=f16(segm2), segm2_S=S2.detach().numpy().astype(np.float32).reshape(1), segm2_d_segm=dS2.numpy())
    for b in range(2):
        arrays['segm2_masks_%d' % b] = masks2[b].numpy().astype(np.uint8)
        arrays['segm2_labels_%d' % b] = labels2[b].numpy().astype(np.int16)
    print('segm2: S = %.6f' % float(S2))

    meta = dict(P=P, pyramid=list(PYRAMID), max_size=MAX_SIZE, num_classes=NUM_CLASSES, num_crowds=num_crowds, gap=GAP,
                negpos_ratio=3, conf_alpha=1.0, semantic_segmentation_alpha=1.0, bbox_alpha=1.5, mask_alpha=6.125,
                torch=torch.__version__)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'multibox.npz')
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < 256 * 1024


if __name__ == '__main__':
    main()
