"""COCO box / mask mAP at engine speed: eval.py's metric mode (prep_metrics, APDataObject, calc_map; eval.py:386-510,
:533-581, :1006-1032) with detections, masks and the bookkeeping on the device.

    ev = APEvaluator(num_classes)
    ev.add(preds, gt, gt_masks, h, w, num_crowd, batch_idx=b)      # per image, what eval.prep_metrics takes
    maps = ev.calc_map()                                           # {'box': OrderedDict, 'mask': OrderedDict}, the reference's table

Per image `add` runs postprocess_bits (masks stay bits), packs the GT masks to bits, computes the four IoU matrices
(csrc/metrics.hip) and launches csrc/ap_eval.hip's match kernel, which appends one record per detection and IoU type: no host
synchronisation, no device -> host read.  `ap_objects` sorts the records once (torch's stable device sort on a packed key) and
runs the AP kernel: APDataObject.get_ap for every (type, threshold, class) in fp64, bit-equal to the reference.  The class means
are taken on the host in the reference's order.

Ground-truth masks are 0/1 (what COCODetection.pull_item returns); crowd GT are the last `num_crowd` rows (eval.py:396-400).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L

IOU_THRESHOLDS = [x / 100 for x in range(50, 100, 5)]      # eval.py:31
IOU_TYPES = ('box', 'mask')


def gt_boxes_px(gt, w, h):
    """eval.py:389-392: torch.Tensor(gt[:, :4]) (float32), x columns *= w, y columns *= h, in float32."""
    b = np.asarray(gt, dtype=np.float64)[:, :4].astype(np.float32)
    b[:, [0, 2]] *= np.float32(w)
    b[:, [1, 3]] *= np.float32(h)
    return b


def calc_map_from_ap(ap, rounded=True):
    """eval.py:1006-1032 from an ap_objects() array [2, 10, num_classes] (NaN = empty object): per type and threshold the
    sequential sum of the non-empty class APs in class order / count * 100; 'all' = (0 + every threshold's value) / 10."""
    ap = np.asarray(ap, dtype=np.float64)
    all_maps = {'box': OrderedDict(), 'mask': OrderedDict()}
    for t, iou_type in enumerate(IOU_TYPES):
        all_maps[iou_type]['all'] = 0
        for i, threshold in enumerate(IOU_THRESHOLDS):
            aps = [float(v) for v in ap[t, i] if not np.isnan(v)]
            all_maps[iou_type][int(threshold * 100)] = sum(aps) / len(aps) * 100 if len(aps) > 0 else 0
        all_maps[iou_type]['all'] = sum(all_maps[iou_type].values()) / (len(all_maps[iou_type].values()) - 1)
    if rounded:
        all_maps = {k: OrderedDict((j, round(u, 2)) for j, u in v.items()) for k, v in all_maps.items()}
    return all_maps


class APData:
    """APDataObject's state (eval.py:519-545), for to_ap_data(): data_points in insertion order, num_gt_positives.  get_ap() is
    the reference's host computation, so that eval.py's calc_map can consume a pickled export (APEvaluator itself never calls it)."""

    def __init__(self):
        self.data_points = []
        self.num_gt_positives = 0

    def push(self, score, is_true):
        self.data_points.append((score, is_true))

    def add_gt_positives(self, num_positives):
        self.num_gt_positives += num_positives

    def is_empty(self):
        return len(self.data_points) == 0 and self.num_gt_positives == 0

    def get_ap(self):
        if self.num_gt_positives == 0:
            return 0
        self.data_points.sort(key=lambda x: -x[0])
        precisions, recalls = [], []
        num_true = num_false = 0
        for _, is_true in self.data_points:
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


def _upload(a, dtype, device):
    """Host array -> device tensor through pinned memory, asynchronously (no host synchronisation)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
    if t.numel() == 0:
        return torch.empty(t.shape, dtype=t.dtype, device=device)
    return t.pin_memory().to(device, non_blocking=True)


class APEvaluator:
    """The ap_data of eval.py's metric mode, held on the device.  See the module docstring."""

    def __init__(self, num_classes, device=None):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError('APEvaluator: num_classes must be >= 1')
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.type != 'cuda':
            raise RuntimeError('APEvaluator: the evaluator runs on the GPU (MI355X/HIP); there is no CPU path')
        self.reset()

    def reset(self):
        self._n = 0                 # records per type so far
        self._cap = 0
        self._key = self._score = self._flags = None
        self._gt_count = torch.zeros(self.num_classes, dtype=torch.int64, device=self.device)

    def _reserve(self, extra):
        need = self._n + extra
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, 4096)
        key = torch.empty(2, cap, dtype=torch.int64, device=self.device)
        score = torch.empty(2, cap, dtype=torch.float32, device=self.device)
        flags = torch.empty(2, cap, dtype=torch.int32, device=self.device)
        if self._n:
            key[:, :self._n].copy_(self._key[:, :self._n])
            score[:, :self._n].copy_(self._score[:, :self._n])
            flags[:, :self._n].copy_(self._flags[:, :self._n])
        self._key, self._score, self._flags, self._cap = key, score, flags, cap

    def add(self, dets_out, gt, gt_masks, h, w, num_crowd, batch_idx=0, crop_masks=True, score_threshold=0):
        """eval.prep_metrics (metric mode) for image `batch_idx` of `dets_out` (Yolact.forward's output).  score_threshold > 0
        filters the detections with a boolean mask, which reads the count back like postprocess does."""
        from .layers.output_utils import postprocess_bits
        classes, scores, boxes, bits = postprocess_bits(dets_out, w, h, batch_idx=batch_idx, crop_masks=crop_masks,
                                                        score_threshold=score_threshold)
        if bits is None:
            return                                  # eval.py:405-406
        self.add_detections(classes, scores, boxes, bits, gt, gt_masks, h, w, num_crowd)

    def add_detections(self, classes, scores, boxes_px, mask_bits, gt, gt_masks, h, w, num_crowd):
        """The same from postprocessed device tensors: classes [N] int, scores [N] (or the YOLACT++ [box_scores, mask_scores]),
        boxes_px [N,4] integer pixels, mask_bits int64 [N, ceil(h*w/64)] (output_utils.postprocess_bits / box_utils.mask_bits);
        gt [n,5] relative xyxy + class (host), gt_masks [n,h,w] 0/1 (host, or a device tensor, which stays there), crowds last."""
        if isinstance(classes, (list, tuple)) or classes.shape[0] == 0:
            return                                  # eval.py:405-406: the GT of an image without detections is not counted
        N = int(classes.shape[0])
        if N > L.AP_MAX_DET:
            raise RuntimeError('APEvaluator: %d detections in one image (at most %d)' % (N, L.AP_MAX_DET))
        box_scores, mask_scores = (scores[0], scores[1]) if isinstance(scores, (list, tuple)) else (scores, scores)
        dev = classes.device
        L.require_cuda(classes, 'classes')
        gt = np.zeros((0, 5)) if gt is None else np.asarray(gt, dtype=np.float64).reshape(-1, 5)
        num_crowd = int(num_crowd)
        n_all = gt.shape[0]
        G = n_all - num_crowd
        if num_crowd < 0 or G < 0:
            raise ValueError('APEvaluator: num_crowd %d with %d GT rows' % (num_crowd, n_all))
        if G > L.AP_MAX_GT or num_crowd > L.AP_MAX_GT:
            raise RuntimeError('APEvaluator: %d GT / %d crowd regions in one image (at most %d each)' % (G, num_crowd, L.AP_MAX_GT))
        gt_cls = gt[:, 4].astype(int)
        if G and (gt_cls[:G].min() < 0 or gt_cls[:G].max() >= self.num_classes):
            raise ValueError('APEvaluator: GT class outside [0, %d)' % self.num_classes)
        n = h * w
        W64 = (n + 63) // 64
        if mask_bits.shape[1] != W64:
            raise RuntimeError('APEvaluator: mask_bits has %d words per mask, %d x %d needs %d' % (mask_bits.shape[1], h, w, W64))
        self._reserve(N)
        lib = L.lib()
        with torch.cuda.device(dev):
            s = L.stream_ptr()
            cls_d = classes.contiguous().long()
            bs = box_scores.contiguous().float()
            ms = mask_scores.contiguous().float() if mask_scores is not box_scores else bs
            det_boxes = boxes_px.contiguous().float()
            det_bits = mask_bits.contiguous()
            boxes_d = _upload(gt_boxes_px(gt, w, h), np.float32, dev)
            cls_gt = _upload(gt_cls, np.int32, dev)
            ious = [None] * 4                       # box, mask, crowd box, crowd mask
            if n_all:
                if torch.is_tensor(gt_masks) and gt_masks.is_cuda:      # COCODetection(device_masks=True): used where they are
                    gm_f = gt_masks.to(dev).reshape(n_all, n).to(torch.uint8).float()
                else:
                    gm = gt_masks.cpu().numpy() if torch.is_tensor(gt_masks) else np.asarray(gt_masks)
                    gm_f = _upload(gm.reshape(n_all, n), np.uint8, dev).float()
                gt_bits = torch.empty(n_all, W64, dtype=torch.int64, device=dev)
                L.check(lib.ymi_mask_bits_f32(gm_f.data_ptr(), n_all, n, gt_bits.data_ptr(), s), 'ymi_mask_bits_f32')
                for slot, lo, hi, crowd in ((0, 0, G, 0), (2, G, n_all, 1)):
                    if hi == lo:
                        continue
                    bi = torch.empty(N, hi - lo, dtype=torch.float32, device=dev)
                    mi = torch.empty(N, hi - lo, dtype=torch.float32, device=dev)
                    L.check(lib.ymi_jaccard_f32(det_boxes.data_ptr(), boxes_d[lo:hi].data_ptr(), N, hi - lo, crowd, bi.data_ptr(), s),
                            'ymi_jaccard_f32')
                    L.check(lib.ymi_mask_iou_bits(det_bits.data_ptr(), gt_bits[lo:hi].data_ptr(), N, hi - lo, W64, crowd, mi.data_ptr(), s),
                            'ymi_mask_iou_bits')
                    ious[slot], ious[slot + 1] = bi, mi
            ptr = lambda t: t.data_ptr() if t is not None else None
            d = L.ApMatchDesc()
            d.cls, d.box_score, d.mask_score = cls_d.data_ptr(), bs.data_ptr(), ms.data_ptr()
            d.box_iou, d.mask_iou, d.crowd_box_iou, d.crowd_mask_iou = (ptr(t) for t in ious)
            d.gt_cls = cls_gt.data_ptr() if G else None
            d.crowd_cls = cls_gt[G:].data_ptr() if num_crowd else None
            d.rec_key, d.rec_score, d.rec_flags = self._key.data_ptr(), self._score.data_ptr(), self._flags.data_ptr()
            d.gt_count = self._gt_count.data_ptr()
            d.base, d.cap = self._n, self._cap
            d.N, d.G, d.Gc, d.num_classes = N, G, num_crowd, self.num_classes
            L.check(lib.ymi_ap_match_f32(C.byref(d), s), 'ymi_ap_match_f32')
        self._n += N

    def ap_objects(self):
        """float64 [2, 10, num_classes]: APDataObject.get_ap() of ap_data[type][threshold][class], NaN where is_empty()."""
        M, nc = self._n, self.num_classes
        with torch.cuda.device(self.device):
            ap = torch.empty(2, L.AP_NUM_THRESH, nc, dtype=torch.float64, device=self.device)
            empty = torch.empty(2, L.AP_NUM_THRESH, nc, dtype=torch.int32, device=self.device)
            d = L.ApFinalizeDesc()
            if M:
                sorted_key, perm = torch.sort(self._key[:, :M], dim=1, stable=True)
                d.sorted_key, d.perm, d.rec_flags = sorted_key.data_ptr(), perm.data_ptr(), self._flags.data_ptr()
            d.gt_count, d.ap, d.empty = self._gt_count.data_ptr(), ap.data_ptr(), empty.data_ptr()
            d.M, d.cap, d.num_classes = M, self._cap, nc
            L.check(L.lib().ymi_ap_finalize_f64(C.byref(d), L.stream_ptr()), 'ymi_ap_finalize_f64')
            out = ap.cpu().numpy()
            out[empty.cpu().numpy() != 0] = np.nan
        return out

    def calc_map(self, rounded=True):
        """eval.calc_map: {'box': OrderedDict, 'mask': OrderedDict} with keys 'all', 50, 55, ..., 95 (rounded to 2 decimals
        like eval.py:1030 unless rounded=False)."""
        return calc_map_from_ap(self.ap_objects(), rounded)

    def to_ap_data(self):
        """The reference's ap_data: {'box': [[APData] * num_classes] * 10, 'mask': ...}, data_points in insertion order."""
        M = self._n
        key = self._key[:, :M].cpu().numpy() if M else np.zeros((2, 0), np.int64)
        score = self._score[:, :M].cpu().numpy() if M else np.zeros((2, 0), np.float32)
        flags = self._flags[:, :M].cpu().numpy() if M else np.zeros((2, 0), np.int32)
        ngt = self._gt_count.cpu().numpy()
        out = {t: [[APData() for _ in range(self.num_classes)] for _ in IOU_THRESHOLDS] for t in IOU_TYPES}
        for t, name in enumerate(IOU_TYPES):
            for k in range(len(IOU_THRESHOLDS)):
                sel = np.nonzero((flags[t] >> (16 + k)) & 1)[0]
                cls = key[t, sel] >> 32
                order = np.argsort(cls, kind='stable')                 # per class, insertion order kept
                sel, cls = sel[order], cls[order]
                bounds = np.searchsorted(cls, np.arange(self.num_classes + 1))
                sc = score[t, sel].astype(np.float64).tolist()
                tp = (((flags[t, sel] >> k) & 1) != 0).tolist()
                for c, obj in enumerate(out[name][k]):
                    obj.num_gt_positives = int(ngt[c])
                    obj.data_points = list(zip(sc[bounds[c]:bounds[c + 1]], tp[bounds[c]:bounds[c + 1]]))
        return out


def evaluate(net, dataset, batch_size=8, max_images=None, crop_masks=True, score_threshold=0):
    """eval.py:930-993 in metric mode: dataset.pull_item in dataset order, one forward per batch, APEvaluator.add per image;
    returns calc_map() (rounded).  Prints nothing."""
    from .config import active_cfg
    ev = APEvaluator(active_cfg().num_classes - 1)             # len(cfg.dataset.class_names): the classes without background
    n = len(dataset) if max_images is None else min(int(max_images), len(dataset))
    for s in range(0, n, batch_size):
        items = [dataset.pull_item(i) for i in range(s, min(s + batch_size, n))]
        with torch.no_grad():
            preds = net(torch.stack([it[0] for it in items]).to(ev.device))
            for b, (_, gt, gt_masks, h, w, num_crowd) in enumerate(items):
                ev.add(preds, gt, gt_masks, h, w, num_crowd, batch_idx=b, crop_masks=crop_masks, score_threshold=score_threshold)
    return ev.calc_map()
