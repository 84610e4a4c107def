"""The lincomb mask loss as a formula, on the CPU, in any dtype (fp64 = the oracle of tests/test_gpu_mask_loss.py; fp32 = the
yardstick of its bar).  Differentiable torch operations only; F.binary_cross_entropy itself supplies the clamped logs (a hand-written
clamp(log(q)) has NaN gradients at q = 0).

    x = sum_k proto[b,r,c,k] coef[j,k]    p = sigmoid(x)    q = inside ? p : 0    l = BCE(q, t)    L_j = sum l
    roi_norm: L_j = L_j / ((b2 - b0) mw) / ((b3 - b1) mh) * (crop ? mh mw : 1)     loss = alpha / mh / mw * sum_j weight_j L_j
"""
import torch
import torch.nn.functional as F


def crop_windows(box, mh, mw, dtype):
    """[N,4] (x1, x2, y1, y2) of sanitize_coordinates(padding=1, cast=False) evaluated in `dtype` (box_utils.py:328-346)."""
    b = box.detach().to(dtype)
    ax, cx = b[:, 0] * mw, b[:, 2] * mw
    ay, cy = b[:, 1] * mh, b[:, 3] * mh
    x1 = torch.clamp(torch.min(ax, cx) - 1, min=0)
    x2 = torch.clamp(torch.max(ax, cx) + 1, max=mw)
    y1 = torch.clamp(torch.min(ay, cy) - 1, min=0)
    y2 = torch.clamp(torch.max(ay, cy) + 1, max=mh)
    return torch.stack([x1, x2, y1, y2], 1)


def inside_masks(box, mh, mw, dtype):
    """bool [N,mh,mw]: the pixels crop() keeps (box_utils.py:350-373)."""
    w = crop_windows(box, mh, mw, dtype)
    cols = torch.arange(mw, dtype=dtype).view(1, 1, mw)
    rows = torch.arange(mh, dtype=dtype).view(1, mh, 1)
    x1, x2, y1, y2 = (w[:, i].view(-1, 1, 1) for i in range(4))
    return (cols >= x1) & (cols < x2) & (rows >= y1) & (rows < y2)


def logits(proto, coef, img_off, dtype=torch.float64):
    """[N,mh,mw] x of every instance."""
    B, mh, mw, K = proto.shape
    off = [int(v) for v in img_off]
    out = [torch.einsum('rck,jk->jrc', proto[b].to(dtype), coef[off[b]:off[b + 1]].to(dtype)) for b in range(B)]
    return torch.cat(out) if out else proto.new_zeros(0, mh, mw, dtype=dtype)


def mask_loss_ref(proto, coef, box, gt, gt_idx, img_off, weight, crop=True, roi_norm=True, alpha=6.125, dtype=torch.float64):
    """-> (loss 0-dim, loss_inst [N]) in `dtype`, differentiable in proto and coef."""
    B, mh, mw, K = proto.shape
    N = coef.shape[0]
    if N == 0:
        z = proto.to(dtype).sum() * 0
        return z, torch.zeros(0, dtype=dtype)
    x = logits(proto, coef, img_off, dtype)
    p = torch.sigmoid(x)
    if crop:
        p = p * inside_masks(box, mh, mw, dtype).to(dtype)
    t = gt[gt_idx.long()].ne(0).to(dtype)
    pre = F.binary_cross_entropy(torch.clamp(p, 0, 1), t, reduction='none').sum(dim=(1, 2))
    if roi_norm:
        b = box.detach().to(dtype)
        pre = pre / ((b[:, 2] - b[:, 0]) * mw) / ((b[:, 3] - b[:, 1]) * mh) * (mh * mw if crop else 1)
    loss = (pre * weight.detach().to(dtype)).sum() * alpha / mh / mw
    return loss, pre


def mask_loss_ref_grads(proto, coef, box, gt, gt_idx, img_off, weight, crop=True, roi_norm=True, alpha=6.125, dtype=torch.float64):
    """-> (loss, loss_inst, d_proto, d_coef), detached, in `dtype`."""
    pl = proto.detach().to(dtype).requires_grad_(True)
    cl = coef.detach().to(dtype).requires_grad_(True)
    loss, inst = mask_loss_ref(pl, cl, box, gt, gt_idx, img_off, weight, crop, roi_norm, alpha, dtype)
    if coef.shape[0] == 0:
        return loss.detach(), inst, torch.zeros_like(pl), torch.zeros_like(cl)
    dp, dc = torch.autograd.grad(loss, [pl, cl])
    return loss.detach(), inst.detach(), dp, dc
