"""Host statement of the reference's mAP evaluator WITH the crowd branch, for the AP-evaluation tests.

prep_metrics = eval.py:386-510 in metric mode (postprocess already applied: the caller passes its outputs), APDataObject =
eval.py:519-581, calc_map = eval.py:1006-1032 without printing; IoUs are layers/box_utils.py:54-80 (jaccard, iscrowd) and :98-113
(mask_iou, iscrowd) on CPU float32, with empty operands giving empty matrices.  The case builders and the fixture's (un)packing
live in tools/make_golden_ap_eval.py, which is loaded from here.
"""
from __future__ import annotations

import functools
import importlib.util
import os
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ap_eval.npz')
IOU_THRESHOLDS = [x / 100 for x in range(50, 100, 5)]


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location('make_golden_ap_eval', os.path.join(ROOT, 'tools', 'make_golden_ap_eval.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def case(name):
    """-> (meta, images) of a golden case; images as tools/make_golden_ap_eval._image dicts."""
    return generator().images_from_arrays(load(), name)


def jaccard(a, b, iscrowd=False):
    if a.shape[0] == 0 or b.shape[0] == 0:
        return torch.zeros(a.shape[0], b.shape[0])
    mx = torch.min(a[:, None, 2:], b[None, :, 2:])
    mn = torch.max(a[:, None, :2], b[None, :, :2])
    inter = torch.clamp(mx - mn, min=0).prod(2)
    area_a = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).unsqueeze(1).expand_as(inter)
    area_b = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).unsqueeze(0).expand_as(inter)
    return inter / area_a if iscrowd else inter / (area_a + area_b - inter)


def mask_iou(a, b, iscrowd=False):
    if a.shape[0] == 0 or b.shape[0] == 0:
        return torch.zeros(a.shape[0], b.shape[0])
    inter = a @ b.t()
    area_a = a.sum(dim=1).unsqueeze(1)
    area_b = b.sum(dim=1).unsqueeze(0)
    return inter / (area_a + area_b - inter) if not iscrowd else inter / area_a


class APDataObject:
    def __init__(self):
        self.data_points = []
        self.num_gt_positives = 0

    def push(self, score, is_true):
        self.data_points.append((score, is_true))

    def add_gt_positives(self, n):
        self.num_gt_positives += n

    def is_empty(self):
        return len(self.data_points) == 0 and self.num_gt_positives == 0

    def get_ap(self):
        if self.num_gt_positives == 0:
            return 0
        pts = sorted(self.data_points, key=lambda x: -x[0])
        precisions, recalls = [], []
        num_true = num_false = 0
        for _, is_true in pts:
            if is_true:
                num_true += 1
            else:
                num_false += 1
            precisions.append(num_true / (num_true + num_false))
            recalls.append(num_true / self.num_gt_positives)
        for i in range(len(precisions) - 1, 0, -1):
            if precisions[i] > precisions[i - 1]:
                precisions[i - 1] = precisions[i]
        y_range = [0] * 101
        indices = np.searchsorted(np.array(recalls), np.array([x / 100 for x in range(101)]), side='left')
        for bar_idx, precision_idx in enumerate(indices):
            if precision_idx < len(precisions):
                y_range[bar_idx] = precisions[precision_idx]
        return sum(y_range) / len(y_range)


def new_ap_data(num_classes):
    return {t: [[APDataObject() for _ in range(num_classes)] for _ in IOU_THRESHOLDS] for t in ('box', 'mask')}


def prep_metrics(ap_data, im):
    """One image (a make_golden_ap_eval image dict) into ap_data, eval.py:386-510."""
    h, w, num_crowd = im['h'], im['w'], im['num_crowd']
    gt = im['gt']
    gt_boxes = torch.Tensor(gt[:, :4])
    gt_boxes[:, [0, 2]] *= w
    gt_boxes[:, [1, 3]] *= h
    gt_classes = list(gt[:, 4].astype(int))
    gt_masks = torch.Tensor(im['gt_masks'].astype(np.float32)).reshape(-1, h * w)
    crowd_classes = []
    if num_crowd > 0:
        split = lambda x: (x[-num_crowd:], x[:-num_crowd])
        crowd_boxes, gt_boxes = split(gt_boxes)
        crowd_masks, gt_masks = split(gt_masks)
        crowd_classes, gt_classes = split(gt_classes)
    if len(im['cls']) == 0:
        return
    classes = list(im['cls'].astype(int))
    box_scores = list(im['score'].astype(float))
    mask_scores = box_scores if im['score2'] is None else list(im['score2'].astype(float))
    masks = torch.from_numpy(im['masks'].astype(np.float32)).reshape(-1, h * w)
    boxes = torch.from_numpy(im['box']).float()
    num_pred, num_gt = len(classes), len(gt_classes)
    mask_iou_cache = mask_iou(masks, gt_masks)
    bbox_iou_cache = jaccard(boxes, gt_boxes.float())
    if num_crowd > 0:
        crowd_mask_iou_cache = mask_iou(masks, crowd_masks, iscrowd=True)
        crowd_bbox_iou_cache = jaccard(boxes, crowd_boxes.float(), iscrowd=True)
    else:
        crowd_mask_iou_cache = crowd_bbox_iou_cache = None
    box_indices = sorted(range(num_pred), key=lambda i: -box_scores[i])
    mask_indices = sorted(box_indices, key=lambda i: -mask_scores[i])
    iou_types = [('box', bbox_iou_cache, crowd_bbox_iou_cache, box_scores, box_indices),
                 ('mask', mask_iou_cache, crowd_mask_iou_cache, mask_scores, mask_indices)]
    for _class in set(classes + gt_classes):
        num_gt_for_class = sum(1 for x in gt_classes if x == _class)
        for iou_idx, iou_threshold in enumerate(IOU_THRESHOLDS):
            for iou_type, iou_cache, crowd_cache, score, indices in iou_types:
                gt_used = [False] * len(gt_classes)
                ap_obj = ap_data[iou_type][iou_idx][_class]
                ap_obj.add_gt_positives(num_gt_for_class)
                for i in indices:
                    if classes[i] != _class:
                        continue
                    max_iou_found, max_match_idx = iou_threshold, -1
                    for j in range(num_gt):
                        if gt_used[j] or gt_classes[j] != _class:
                            continue
                        iou = iou_cache[i, j].item()
                        if iou > max_iou_found:
                            max_iou_found, max_match_idx = iou, j
                    if max_match_idx >= 0:
                        gt_used[max_match_idx] = True
                        ap_obj.push(score[i], True)
                    else:
                        matched_crowd = False
                        for j in range(len(crowd_classes)):
                            if crowd_classes[j] != _class:
                                continue
                            if crowd_cache[i, j].item() > iou_threshold:
                                matched_crowd = True
                                break
                        if not matched_crowd:
                            ap_obj.push(score[i], False)


def ap_array(ap_data):
    """[2, 10, C] get_ap() values, NaN where is_empty()."""
    C = len(ap_data['box'][0])
    out = np.zeros((2, len(IOU_THRESHOLDS), C))
    for t, typ in enumerate(('box', 'mask')):
        for k in range(len(IOU_THRESHOLDS)):
            for c in range(C):
                o = ap_data[typ][k][c]
                out[t, k, c] = np.nan if o.is_empty() else o.get_ap()
    return out


def calc_map(ap_data, rounded=False):
    C = len(ap_data['box'][0])
    aps = [{'box': [], 'mask': []} for _ in IOU_THRESHOLDS]
    for _class in range(C):
        for iou_idx in range(len(IOU_THRESHOLDS)):
            for iou_type in ('box', 'mask'):
                ap_obj = ap_data[iou_type][iou_idx][_class]
                if not ap_obj.is_empty():
                    aps[iou_idx][iou_type].append(ap_obj.get_ap())
    all_maps = {'box': OrderedDict(), 'mask': OrderedDict()}
    for iou_type in ('box', 'mask'):
        all_maps[iou_type]['all'] = 0
        for i, threshold in enumerate(IOU_THRESHOLDS):
            m = sum(aps[i][iou_type]) / len(aps[i][iou_type]) * 100 if len(aps[i][iou_type]) > 0 else 0
            all_maps[iou_type][int(threshold * 100)] = m
        all_maps[iou_type]['all'] = sum(all_maps[iou_type].values()) / (len(all_maps[iou_type].values()) - 1)
    if rounded:
        all_maps = {k: {j: round(u, 2) for j, u in v.items()} for k, v in all_maps.items()}
    return all_maps


def run(imgs, num_classes):
    ap_data = new_ap_data(num_classes)
    for im in imgs:
        prep_metrics(ap_data, im)
    return ap_data


def golden_points(name, t, k, c):
    """The golden data_points of object (type t, threshold k, class c), insertion order."""
    z = load()
    cnt = z[name + '_dp_count']
    off = int(cnt.reshape(-1)[: (t * cnt.shape[1] + k) * cnt.shape[2] + c].sum())
    n = int(cnt[t, k, c])
    return list(zip(z[name + '_dp_score'][off:off + n].tolist(), z[name + '_dp_tp'][off:off + n].tolist()))
