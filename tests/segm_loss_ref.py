"""The semantic segmentation loss 'S' in plain torch, written from the semantics: the oracle of tests/test_segm_loss_host.py
(pinned there to what the reference itself computed) and of tests/test_gpu_segm_loss.py.  Works in the dtype of `segm`.
combine='sum' is a deliberately WRONG variant (two objects of one class add up instead of OR).
"""
import torch


def segm_targets(gt, label, gt_off, B, K, dtype, combine='or'):
    """gt [G,mh,mw] 0 / 1, label [G], gt_off B + 1 offsets -> the [B,K,mh,mw] target."""
    t = torch.zeros(B, K, gt.size(1), gt.size(2), dtype=dtype)
    for b in range(B):
        for g in range(int(gt_off[b]), int(gt_off[b + 1])):
            m = gt[g].ne(0).to(dtype)
            c = int(label[g])
            t[b, c] = torch.max(t[b, c], m) if combine == 'or' else t[b, c] + m
    return t


def segm_ref(segm, gt, label, gt_off, alpha=1.0, combine='or'):
    """-> (loss 0-dim, d_segm): alpha / (mh mw) * the summed BCE with logits in its stable form, and its gradient."""
    B, K, mh, mw = segm.shape
    t = segm_targets(gt, label, gt_off, B, K, segm.dtype, combine)
    x = segm
    # max(x, 0) as (x + |x|) / 2: autograd then gives sigmoid(0) - t = 0.5 - t at x = 0, where clamp's subgradient would be 1 - t
    per = 0.5 * (x + x.abs()) - x * t + torch.log1p(torch.exp(-x.abs()))
    scale = alpha / (mh * mw)
    return scale * per.sum(), scale * (torch.sigmoid(x) - t)
