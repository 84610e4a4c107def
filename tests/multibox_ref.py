"""MultiBoxLoss.forward for B + M + C + S composed from the oracles of its terms (match_ref, mask_loss_ref, class_loss_ref,
segm_loss_ref), in any dtype: the oracle of tests/test_multibox_host.py (pinned there to the reference's own forward) and of
tests/test_gpu_multibox.py.  The matching is always decided in fp32 (its thresholds are fp32 decisions); the losses and the
gradients of their sum are computed by autograd in `dtype`.  s_norm='num_pos' is a deliberately WRONG variant.
"""
import torch
import torch.nn.functional as F

import class_loss_ref as CR
import mask_loss_ref as MR
import match_ref as TR
import segm_loss_ref as SR

NAMES = ('loc', 'conf', 'mask', 'proto', 'segm')


def multibox_ref(preds, targets, masks, num_crowds, dtype=torch.float64, negpos_ratio=3, bbox_alpha=1.5, mask_alpha=6.125,
                 conf_alpha=1.0, segm_alpha=1.0, masks_to_train=100, s_norm='batch'):
    """preds: dict of CPU fp32 tensors (loc, conf, mask, priors, proto, segm) -> (losses {'B','M','C','S'}, grads {name: d sum / d name},
    extras dict(conf_t, neg, num_pos, key, n))."""
    from yolact_amd.layers.mask_loss import gather_instances
    from yolact_amd.layers.segm_loss import downsample_targets
    priors = preds['priors']
    m = TR.match_batch_ref(priors, targets, num_crowds)
    pos, idx_t, conf_t = m['pos'], m['idx_t'], m['conf_t']
    loc_t = torch.stack([TR.encode_ref(g.to(dtype), priors.to(dtype)) for g in m['gt_box_t']])
    leaves = {k: preds[k].detach().to(dtype).requires_grad_(True) for k in NAMES}
    obj_masks = [x[:x.size(0) - nc] for x, nc in zip(masks, num_crowds)]
    labels = [t[:t.size(0) - nc, 4].long() for t, nc in zip(targets, num_crowds)]
    losses = {}
    losses['B'] = F.smooth_l1_loss(leaves['loc'][pos], loc_t[pos], reduction='sum') * bbox_alpha
    mh, mw = preds['proto'].shape[1:3]
    coef, box, gt, gt_idx, img_off, weight, _ = gather_instances(pos, idx_t, leaves['mask'], obj_masks, m['gt_box_t'], mh, mw, masks_to_train)
    losses['M'] = MR.mask_loss_ref(leaves['proto'], coef, box, gt, gt_idx, img_off, weight, alpha=mask_alpha, dtype=dtype)[0]
    c = CR.ohem_ref(leaves['conf'], conf_t, negpos_ratio, conf_alpha)
    losses['C'] = c['loss']
    sh, sw = preds['segm'].shape[2:]
    sgt, slabel, soff = downsample_targets(obj_masks, labels, sh, sw, 'cpu')
    losses['S'] = SR.segm_ref(leaves['segm'], sgt, slabel, soff, segm_alpha)[0]
    total = pos.sum().to(dtype)
    B = preds['loc'].size(0)
    losses = {k: v / (B if (k == 'S' and s_norm == 'batch') else total) for k, v in losses.items()}
    grads = torch.autograd.grad(sum(losses.values()), [leaves[k] for k in NAMES])
    extras = dict(conf_t=conf_t, neg=c['neg'], num_pos=pos.sum(1), key=c['key'].detach(), n=c['n'])
    return {k: v.detach() for k, v in losses.items()}, dict(zip(NAMES, grads)), extras


def golden_forward(G, meta):
    """The forward case of tests/golden/multibox.npz -> (preds, targets, masks, num_crowds)."""
    preds = {k: G['fwd_' + k].float() for k in NAMES}
    preds['priors'] = G['priors']
    B = preds['loc'].size(0)
    targets = [G['fwd_targets_%d' % b] for b in range(B)]
    masks = [G['fwd_masks_%d' % b].float() for b in range(B)]
    return preds, targets, masks, list(meta['num_crowds'])
