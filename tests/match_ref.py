"""MultiBoxLoss target assignment and the box loss in plain torch, written from the semantics (not from the reference's text):
the oracle of tests/test_match_host.py (pinned there to what the reference itself computed) and of tests/test_gpu_match.py.

Everything works in the dtype and on the device of `priors`.  Every arg-max is explicit about ties (the lowest index among equal values); the
keyword switches select deliberately WRONG variants, which the host test shows the golden file tells apart.
"""
import torch

import helpers
from helpers import rel_err  # noqa: F401  (the tests and tools reach it as match_ref.rel_err)

BIG = 1 << 40


def make_priors(sizes, max_size=550):
    """The prior set of yolact_base_config over the pyramid `sizes` (conv sizes per level, at most 5): [P,4] fp32 centre-size."""
    import yolact_amd
    from yolact_amd.config import make_priors_host
    bb = yolact_amd.CONFIGS['yolact_base_config'].backbone
    data = []
    for lvl, s in enumerate(sizes):
        data += make_priors_host(s, s, bb.pred_scales[lvl], bb.pred_aspect_ratios[lvl], max_size, bb)
    return torch.tensor(data, dtype=torch.float32).view(-1, 4)


def argmax_tie(v, dim, tie='lowest'):
    """(max, index) along dim; among equal maxima the lowest (or, wrong on purpose, the highest) index."""
    m = v.max(dim, keepdim=True)[0]
    shape = [1] * v.dim()
    shape[dim] = -1
    ar = torch.arange(v.size(dim), device=v.device).view(shape).expand_as(v)
    if tie == 'lowest':
        idx = torch.where(v == m, ar, torch.full_like(ar, BIG)).min(dim)[0]
    else:
        idx = torch.where(v == m, ar, torch.full_like(ar, -1)).max(dim)[0]
    return m.squeeze(dim), idx


def point_form(priors):
    return torch.cat((priors[:, :2] - priors[:, 2:] / 2, priors[:, :2] + priors[:, 2:] / 2), 1)


def _inter(a, b):
    """[A,4] x [B,4] point form -> [A,B] intersection areas."""
    wh = (torch.min(a[:, None, 2:], b[None, :, 2:]) - torch.max(a[:, None, :2], b[None, :, :2])).clamp(min=0)
    return wh[..., 0] * wh[..., 1]


def _area(a):
    return (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])


def iou(a, b):
    i = _inter(a, b)
    return i / (_area(a)[:, None] + _area(b)[None, :] - i)


def encode_ref(matched, priors):
    """matched [P,4] point form, priors [P,4] centre-size -> regression targets, variances 0.1 / 0.2, in the dtype given."""
    v0 = torch.tensor(0.1, dtype=priors.dtype, device=priors.device)
    v1 = torch.tensor(0.2, dtype=priors.dtype, device=priors.device)
    cxcy = ((matched[:, :2] + matched[:, 2:]) / 2 - priors[:, :2]) / (v0 * priors[:, 2:])
    wh = torch.log((matched[:, 2:] - matched[:, :2]) / priors[:, 2:]) / v1
    return torch.cat([cxcy, wh], 1)


def match_ref(priors, truths, labels, crowds, pos_thresh=0.5, neg_thresh=0.4, crowd_thresh=0.7, tie='lowest',
              pos_first=True, crowd_over='prior', forced=True):
    """One image.  priors [P,4] centre-size, truths [n,4] point form, labels [n] long, crowds [c,4] or None
    -> dict(loc_t [P,4], conf_t [P] long, idx_t [P] long, gt_box_t [P,4], pos [P] bool)."""
    dt = priors.dtype
    truths = truths.to(dt)
    boxes = point_form(priors)
    ov = iou(truths, boxes)                                             # [n,P]
    best_ov, best_idx = argmax_tie(ov, 0, tie)
    best_ov = best_ov.clone()
    if forced:
        ov = ov.clone()
        for _ in range(ov.size(0)):
            row_max, row_arg = argmax_tie(ov, 1, tie)
            j = int(argmax_tie(row_max, 0, tie)[1])
            i = int(row_arg[j])
            ov[:, i] = -1
            ov[j, :] = -1
            best_ov[i] = 2
            best_idx[i] = j
    conf = labels[best_idx].long() + 1
    lo, hi = torch.tensor(neg_thresh, dtype=dt, device=priors.device), torch.tensor(pos_thresh, dtype=dt, device=priors.device)
    if pos_first:
        conf[best_ov < hi] = -1
        conf[best_ov < lo] = 0
    else:
        conf[best_ov < lo] = 0
        conf[best_ov < hi] = -1
    if crowds is not None and crowds.size(0) > 0 and crowd_thresh < 1:
        crowds = crowds.to(dt)
        i = _inter(boxes, crowds)                                       # [P,c]
        ratio = i / (_area(boxes)[:, None] if crowd_over == 'prior' else _area(crowds)[None, :])
        conf[(conf <= 0) & (ratio.max(1)[0] > torch.tensor(crowd_thresh, dtype=dt, device=priors.device))] = -1
    gt_box = truths[best_idx]
    return dict(loc_t=encode_ref(gt_box, priors), conf_t=conf, idx_t=best_idx, gt_box_t=gt_box, pos=conf > 0)


def split_targets(targets, num_crowds):
    """The reference's bundled targets -> per image (truths [n,4], labels [n] long, crowds [c,4] or None)."""
    out = []
    for tgt, nc in zip(targets, num_crowds):
        n = tgt.size(0) - nc
        out.append((tgt[:n, :4], tgt[:n, 4].long(), tgt[n:, :4] if nc > 0 else None))
    return out


def match_batch_ref(priors, targets, num_crowds, **kw):
    """match_ref image by image, stacked: loc_t [B,P,4], conf_t, idx_t [B,P] long, gt_box_t [B,P,4], pos [B,P], num_pos [B]."""
    per = [match_ref(priors, t, l, c, **kw) for t, l, c in split_targets(targets, num_crowds)]
    out = {k: torch.stack([p[k] for p in per]) for k in per[0]}
    out['num_pos'] = out['pos'].sum(1)
    return out


def box_loss_ref(loc_data, loc_t, pos, alpha=1.5):
    """alpha * summed smooth-L1 (beta 1) over the positives, and its gradient in loc_data (zero off the positives)."""
    d = loc_data - loc_t
    ad = d.abs()
    per = torch.where(ad < 1, 0.5 * d * d, ad - 0.5)
    m = pos.unsqueeze(-1).expand_as(d)
    zero = torch.zeros_like(d)
    loss = alpha * torch.where(m, per, zero).sum()
    return loss, torch.where(m, alpha * d.clamp(-1, 1), zero)


def load_golden():
    """tests/golden/match.npz (tools/make_golden_match.py: the reference's own results) -> (meta, {case name: dict of tensors});
    'targets' is the list of bundled [n,5] tensors, conf_t / idx_t are long."""
    meta, z = helpers.load_golden('match')
    cases = {}
    for c in meta['cases']:
        t = {k: torch.tensor(z['%s_%s' % (c['name'], k)]) for k in ('priors', 'loc_data', 'loc_t', 'conf_t', 'idx_t', 'gt_box_t',
                                                                         'B', 'd_loc')}
        t['conf_t'], t['idx_t'] = t['conf_t'].long(), t['idx_t'].long()
        t['targets'] = [torch.tensor(z['%s_targets_%d' % (c['name'], b)]) for b in range(c['B'])]
        t['num_crowds'] = list(c['num_crowds'])
        cases[c['name']] = t
    return meta, cases
