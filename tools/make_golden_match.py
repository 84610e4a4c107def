"""Generate tests/golden/match.npz by EXECUTING THE REFERENCE's MultiBoxLoss.forward on the CPU (build container only).

    python tools/make_golden_match.py                # needs the reference checkout; writes tests/golden/match.npz

The reference is imported with the stubs of oracle/make_golden._shim_reference under yolact_base_config.  forward() runs its real
target assignment (layers/box_utils.py match, the loop of multibox_loss.py:100-126) and its box loss (:141-145); the terms after
them (mask, class, segmentation) are replaced by zeros, and the stand-in for the class term reads what forward() holds at that
point: gt_box_t and losses['B'] before the normalisation of :196-203.  loc_t, conf_t and idx_t are the tensors match() filled.
Per case the file holds the inputs (priors, the bundled targets, num_crowds, loc_data) and loc_t, conf_t, idx_t, gt_box_t, 'B'
and d B / d loc_data.  Only data is stored.
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

MAX_SIZE = 138                                        # anchors of 0.17, 0.35, 0.70 of the image on the shrunken pyramids below
SMALL, LARGE = (9, 5, 3), (18, 9, 5)                  # 345 and 1290 priors: neither a multiple of the 256-prior tile


def anchor_box(priors, i, shrink):
    """The point-form box of prior i, shrunk about its centre: IoU shrink^2 with that prior."""
    cx, cy, w, h = [float(v) for v in priors[i]]
    return [cx - shrink * w / 2, cy - shrink * h / 2, cx + shrink * w / 2, cy + shrink * h / 2]


def random_targets(g, n, n_crowd=0):
    """n GT boxes the size of the anchors (so that some priors pass 0.5) + n_crowd crowd boxes, bundled as the reference does."""
    size = torch.tensor([0.17, 0.35, 0.70])[torch.randint(0, 3, (n,), generator=g)] * (0.7 + 0.7 * torch.rand(n, generator=g))
    ar = 0.7 + 0.6 * torch.rand(n, generator=g)
    w, h = size * ar, size / ar
    c = 0.1 + 0.8 * torch.rand(n, 2, generator=g)
    box = torch.stack([c[:, 0] - w / 2, c[:, 1] - h / 2, c[:, 0] + w / 2, c[:, 1] + h / 2], 1).clamp(0.0, 1.0)
    cls = torch.randint(0, 80, (n, 1), generator=g).float()
    rows = [torch.cat([box, cls], 1)]
    for _ in range(n_crowd):
        c = 0.2 + 0.6 * torch.rand(2, generator=g)
        half = 0.15 + 0.2 * torch.rand(2, generator=g)
        rows.append(torch.cat([(c - half).clamp(0, 1), (c + half).clamp(0, 1), torch.tensor([-1.0])]).view(1, 5))
    return torch.cat(rows)


def build_cases():
    from match_ref import make_priors
    small, large = make_priors(SMALL, MAX_SIZE), make_priors(LARGE, MAX_SIZE)
    g = torch.Generator().manual_seed(20)
    row = lambda box, cls: torch.tensor([box + [float(cls)]], dtype=torch.float32)
    cases = []
    # (a) 3 GTs, no crowd
    cases.append(('plain3', small, [random_targets(g, 3)], [0]))
    # (b) two GTs whose best prior is the same prior (IoU 0.81 and 0.64 with prior 100): the second row is recomputed
    cases.append(('shared_best', small, [torch.cat([row(anchor_box(small, 100, 0.8), 7), row(anchor_box(small, 100, 0.9), 3),
                                                     random_targets(g, 1)])], [0]))
    # (c) two identical GTs and a zero-area GT (rows whose remaining maximum is 0 take the lowest live column)
    dup = anchor_box(small, 200, 0.85)
    cases.append(('degenerate', small, [torch.cat([row([0.5, 0.5, 0.5, 0.5], 1), row(dup, 5), row(dup, 9)])], [0]))
    # (d) crowds.  image 0: a GT inside a crowd box that covers the left half (its positives stay positive, the background
    # priors inside turn neutral); image 1: no crowd; image 2: random with two crowds
    img0 = torch.cat([row(anchor_box(small, 3 * (9 * 4 + 2), 0.9), 11), row([0.6, 0.1, 0.95, 0.5], 2),
                      row([0.0, 0.0, 0.5, 1.0], -1)])
    cases.append(('crowds', small, [img0, random_targets(g, 4), random_targets(g, 5, 2)], [1, 0, 2]))
    # (e) more GTs than the kernel stages in LDS at once (64), on the larger prior set
    cases.append(('many_gt', large, [random_targets(g, 70, 1)], [1]))
    return cases


def run_reference(crit, mod, priors, targets, num_crowds, loc_data):
    B, P = len(targets), priors.size(0)
    seen = {}
    real_match = mod.match

    def match(pos_thresh, neg_thresh, truths, pri, labels, crowd_boxes, loc_t, conf_t, idx_t, idx, loc):
        seen.update(loc_t=loc_t, conf_t=conf_t, idx_t=idx_t)
        return real_match(pos_thresh, neg_thresh, truths, pri, labels, crowd_boxes, loc_t, conf_t, idx_t, idx, loc)

    def class_term(*a, **k):
        frame = sys._getframe(1).f_locals                          # forward() at multibox_loss.py:184
        seen['gt_box_t'] = frame['gt_box_t'].clone()
        seen['B'] = frame['losses']['B'].clone()                   # before the in-place normalisation of :196-203
        return torch.zeros(())

    zero = lambda *a, **k: torch.zeros(())
    crit.lincomb_mask_loss = lambda *a, **k: {'M': torch.zeros(())}
    crit.ohem_conf_loss = class_term
    crit.semantic_segmentation_loss = zero
    loc = loc_data.clone().requires_grad_(True)
    preds = dict(loc=loc, conf=torch.zeros(B, P, 81), mask=torch.zeros(B, P, 32), priors=priors, proto=torch.zeros(B, 4, 4, 32),
                 segm=torch.zeros(B, 80, 4, 4))
    masks = [torch.zeros(t.size(0), 4, 4) for t in targets]
    mod.match = match
    try:
        crit(None, preds, [t.clone() for t in targets], masks, list(num_crowds))
    finally:
        mod.match = real_match
    (d_loc,) = torch.autograd.grad(seen['B'], [loc])
    return seen['loc_t'], seen['conf_t'], seen['idx_t'], seen['gt_box_t'], seen['B'].detach(), d_loc


def main():
    from oracle.make_golden import _shim_reference
    _shim_reference()
    from data import cfg, set_cfg
    set_cfg('yolact_base_config')
    import layers.modules.multibox_loss as mod
    assert not cfg.use_prediction_matching and not cfg.use_change_matching and not cfg.use_yolo_regressors and cfg.train_boxes
    assert (cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.crowd_iou_threshold, cfg.bbox_alpha) == (0.5, 0.4, 0.7, 1.5)
    assert not cfg.use_focal_loss and not cfg.use_objectness_score and not cfg.use_maskiou and cfg.mask_proto_loss is None
    crit = mod.MultiBoxLoss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, 3)
    arrays, metas = {}, []
    g = torch.Generator().manual_seed(21)
    for name, priors, targets, num_crowds in build_cases():
        B, P = len(targets), priors.size(0)
        loc_data = torch.randn(B, P, 4, generator=g) * 0.7
        loc_t, conf_t, idx_t, gt_box_t, lossB, d_loc = run_reference(crit, mod, priors, targets, num_crowds, loc_data)
        arrays.update({name + '_priors': priors.numpy(), name + '_loc_data': loc_data.numpy(), name + '_loc_t': loc_t.numpy(),
                       name + '_conf_t': conf_t.numpy().astype(np.int16), name + '_idx_t': idx_t.numpy().astype(np.int16),
                       name + '_gt_box_t': gt_box_t.numpy(), name + '_B': lossB.numpy().astype(np.float32).reshape(1),
                       name + '_d_loc': d_loc.numpy()})
        for b, t in enumerate(targets):
            arrays['%s_targets_%d' % (name, b)] = t.numpy()
        metas.append(dict(name=name, B=B, P=P, num_crowds=list(num_crowds), n=[int(t.size(0)) for t in targets]))
        print('%-12s P %4d  n %s crowds %s  positives %s neutral %s  B = %s'
              % (name, P, metas[-1]['n'], list(num_crowds), (conf_t > 0).sum(1).tolist(), (conf_t < 0).sum(1).tolist(), float(lossB)))
    meta = dict(cases=metas, pos_thresh=0.5, neg_thresh=0.4, crowd_thresh=0.7, bbox_alpha=1.5, torch=torch.__version__)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'match.npz')
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
