"""The OHEM class loss 'C' in plain torch, written from the semantics (not from the reference's text): the oracle of
tests/test_class_loss_host.py (pinned there to what the reference itself computed, tests/golden/multibox.npz) and of
tests/test_gpu_class_loss.py.  Works in the dtype of `conf` (fp64 = the oracle, fp32 = the yardstick of the bars).

Two definitions are explicit where the reference is loose: the key is logsumexp(row) - row[0] with the ROW's own maximum
(torch.logsumexp), and equal keys are ranked by prior index, the lowest first (a stable descending sort).  The keyword switches
select deliberately WRONG variants, which the host test shows the golden file tells apart.
"""
import torch

import helpers
from helpers import rel_err  # noqa: F401  (the tests and tools reach it as class_loss_ref.rel_err)


def ohem_ref(conf, conf_t, ratio=3, alpha=1.0, key='lse', zero_pos=True, mine_neutrals=False, ratio_after_clamp=False):
    """conf [B,P,C], conf_t [B,P] long -> dict(loss 0-dim, neg [B,P] bool, num_neg [B], n [B] (marked per image), d_conf [B,P,C],
    key [B,P], lse [B,P])."""
    B, P, C = conf.shape
    pos, neutral = conf_t > 0, conf_t < 0
    lse = torch.logsumexp(conf, 2)
    if key == 'lse':
        k = lse - conf[..., 0]
    else:                                               # wrong on purpose: ohem_use_most_confident's key
        k = torch.softmax(conf, 2)[..., 1:].max(2)[0]
    k = k.clone()
    if zero_pos:
        k[pos] = 0
    if not mine_neutrals:
        k[neutral] = 0
    num_pos = pos.sum(1)
    n = ratio * num_pos.clamp(max=P - 1) if ratio_after_clamp else (ratio * num_pos).clamp(max=P - 1)
    order = torch.sort(k, dim=1, descending=True, stable=True)[1]           # equal keys: the lowest prior first
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(P, device=k.device).expand(B, P).contiguous())
    neg = (rank < n[:, None]) & ~pos
    if not mine_neutrals:
        neg &= ~neutral
    sel = pos | neg
    tgt = conf_t.clamp(min=0)
    term = lse - conf.gather(2, tgt[..., None]).squeeze(2)
    loss = alpha * torch.where(sel, term, torch.zeros_like(term)).sum()
    d = alpha * (torch.softmax(conf, 2) - torch.nn.functional.one_hot(tgt, C).to(conf.dtype))
    d = torch.where(sel[..., None].expand_as(d), d, torch.zeros_like(d))
    return dict(loss=loss, neg=neg, num_neg=neg.sum(1), n=n, d_conf=d, key=k, lse=lse)


def cut_gaps(key, n):
    """Per image the gap between the last marked and the first unmarked key (inf where nothing or everything is marked, or where
    both sides of the cut are 0: positives and neutrals, which are dropped whichever is marked)."""
    s = torch.sort(key, 1, descending=True)[0]
    out = []
    for b in range(key.size(0)):
        m = int(n[b])
        if m <= 0 or m >= key.size(1) or (s[b, m - 1] == 0 and s[b, m] == 0):
            out.append(float('inf'))
        else:
            out.append(float(s[b, m - 1] - s[b, m]))
    return out


def open_the_cuts(conf, conf_t, ratio=3, gap=1e-3):
    """conf with row[0] of the first unmarked row raised where needed, so that every image's cut has a gap of at least `gap`
    (raising row[0] lowers lse - row[0]).  Cases are changed, never dropped."""
    conf = conf.clone()
    for _ in range(64):
        r = ohem_ref(conf.double(), conf_t, ratio)
        gaps = cut_gaps(r['key'], r['n'])
        if min(gaps) >= gap:
            return conf
        order = torch.sort(r["key"], dim=1, descending=True, stable=True)[1]
        for b, g in enumerate(gaps):
            if g < gap:
                conf[b, order[b, int(r["n"][b])], 0] += 0.0625
    raise AssertionError('could not open the cuts')


def load_golden():
    """tests/golden/multibox.npz (tools/make_golden_multibox.py: the reference's own results) -> (meta, dict of tensors)."""
    meta, z = helpers.load_golden('multibox')
    return meta, {k: torch.tensor(v) for k, v in z.items()}
