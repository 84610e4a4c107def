"""Host statement of the reference's traditional (greedy, per-class) NMS Detect, for the traditional-NMS tests.

`greedy_nms` is the fp32 numpy routine tools/make_golden_traditional_nms.py registers in place of the reference's Cython module;
`detect_image` is detection.py:80-108,182-228 around it (candidates, pixel scale, merge, cut), with the device's tie rule.
"""
from __future__ import annotations

import functools
import importlib.util
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'traditional_nms.npz')


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location('make_golden_traditional_nms',
                                                  os.path.join(ROOT, 'tools', 'make_golden_traditional_nms.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def greedy_nms(dets, thresh):
    return generator().greedy_nms(dets, thresh)


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(GOLDEN)
    arrays = {k: z[k] for k in z.files}
    meta = json.loads(bytes(arrays.pop('meta')).decode())
    return meta, arrays


def case(name):
    meta, arrays = load()
    m = [c for c in meta['cases'] if c['name'] == name][0]
    return m, arrays


def golden_image(name, b):
    """The reference's detections of image b: dict(box, mask, class, score, prior) or None."""
    m, arrays = case(name)
    if m['images'][b]['n'] == 0:
        return None
    k = '%s_%d_' % (name, b)
    return {'box': torch.from_numpy(arrays[k + 'box']), 'mask': torch.from_numpy(arrays[k + 'coef']),
            'class': torch.from_numpy(arrays[k + 'class']), 'score': torch.from_numpy(arrays[k + 'score']),
            'prior': torch.from_numpy(arrays[k + 'prior'])}


def decode(loc, priors):
    """box_utils.py:304-310 in fp32, left to right."""
    xy = priors[:, :2] + loc[:, :2] * 0.1 * priors[:, 2:]
    wh = priors[:, 2:] * torch.exp(loc[:, 2:] * 0.2)
    x1y1 = xy - wh / 2
    return torch.cat([x1y1, wh + x1y1], 1)


def detect_image(conf, loc, mask, priors, conf_thresh, nms_thresh, max_det, max_size):
    """conf [P,C] post-softmax -> None or dict(box, mask, class, score, prior); ties: score desc, class asc, prior asc."""
    boxes = decode(loc.float(), priors.float()) * max_size
    cur = conf[:, 1:].t().float()
    cls_l, pri_l, sc_l = [], [], []
    for c in range(cur.shape[0]):
        idx = torch.nonzero(cur[c] > conf_thresh).squeeze(1)
        if idx.numel() == 0:
            continue
        dets = torch.cat([boxes[idx], cur[c, idx][:, None]], 1).numpy()
        keep = torch.from_numpy(greedy_nms(dets, nms_thresh)).long()
        pri_l.append(idx[keep])
        cls_l.append(torch.full((keep.numel(),), c, dtype=torch.int64))
        sc_l.append(cur[c, idx[keep]])
    if not sc_l:
        return None
    pri, cls, sc = torch.cat(pri_l), torch.cat(cls_l), torch.cat(sc_l)
    order = sorted(range(sc.numel()), key=lambda i: (-float(sc[i]), int(cls[i]), int(pri[i])))[:max_det]
    order = torch.tensor(order, dtype=torch.long)
    pri = pri[order]
    return {'box': boxes[pri] / max_size, 'mask': mask[pri], 'class': cls[order], 'score': sc[order], 'prior': pri}


def tie_groups_equal(got_prior, got_class, ref_prior, ref_class, ref_score):
    """Index-exact comparison of two detection lists, order free only inside groups of exactly tied reference scores."""
    gp, gc, rp, rc = (list(map(int, v)) for v in (got_prior, got_class, ref_prior, ref_class))
    rs = [float(v) for v in ref_score]
    if len(gp) != len(rp):
        return False
    i = 0
    while i < len(rp):
        j = i + 1
        while j < len(rp) and rs[j] == rs[i]:
            j += 1
        if sorted(zip(gp[i:j], gc[i:j])) != sorted(zip(rp[i:j], rc[i:j])):
            return False
        i = j
    return True
