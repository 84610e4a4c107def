"""Generate tests/golden/ap_eval.npz by EXECUTING THE REFERENCE'S OWN EVALUATOR (needs the reference checkout).

    python tools/make_golden_ap_eval.py          # needs the reference checkout; writes tests/golden/ap_eval.npz

For every case below a sequence of images (detections + ground truth, built here from a seed) is scored by the reference's
eval.prep_metrics (eval.py:386-510, crowd branch included), APDataObject (eval.py:519-581) and calc_map (eval.py:1006-1032), with
eval.postprocess replaced by a stub that returns the stored detections, exactly as oracle/make_golden_map.py does it.  Recorded,
unrounded: every object's get_ap() (NaN where is_empty()), its data_points in insertion order, its num_gt_positives, and the
calc_map table (also rounded, as calc_map returns it).

Cases (the exact semantics yolact_amd/evaluation.py reproduces):
  thresholds  IoUs equal to the fractions at every threshold and their nearest fp32 neighbours (0.55, 0.7 ... are not fp32
              values), two GT with equal IoU (the first j wins), greedy order;
  crowd       unmatched detections against crowd regions of the class / of another class / of class -1, crowd IoU at and
              around the threshold, matched at low thresholds and crowd-suppressed at high ones;
  edges       empty predicted masks and zero-area boxes (NaN IoUs), images whose GT are all crowd (G = 0) or none (Gc = 0),
              images without detections (their GT are not counted), classes with only detections / only GT;
  ties        score ties inside images and across images, mask-score ties that fall back to the box order, scores <= 0 and
              -0.0 vs +0.0, single- and two-score images;
  many        300 small random images: accumulation and ties across images.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NUM_CLASSES = 80
CASE_NAMES = ['thresholds', 'crowd', 'edges', 'ties', 'many']
FRACTIONS = [(1, 2), (11, 20), (3, 5), (13, 20), (7, 10), (3, 4), (4, 5), (17, 20), (9, 10), (19, 20)]


def _image(h, w, cls, score, box, masks, gt, gt_masks, num_crowd, score2=None):
    n = len(cls)
    return {'h': h, 'w': w, 'cls': np.asarray(cls, np.int64).reshape(n), 'score': np.asarray(score, np.float32).reshape(n),
            'score2': None if score2 is None else np.asarray(score2, np.float32).reshape(n),
            'box': np.asarray(box, np.int64).reshape(n, 4), 'masks': np.asarray(masks, np.uint8).reshape(n, h, w),
            'gt': np.asarray(gt, np.float64).reshape(-1, 5), 'gt_masks': np.asarray(gt_masks, np.uint8).reshape(-1, h, w),
            'num_crowd': int(num_crowd)}


def _strip(h, w, lo, hi):
    m = np.zeros(h * w, np.uint8)
    m[lo:hi] = 1
    return m.reshape(h, w)


def _near_fp32(t, max_den):
    """The fractions a / b (b <= max_den) whose fp32 values lie closest to fp32(t) from below and from above."""
    f = np.float32(t)
    lo = hi = None
    for b in range(2, max_den + 1):
        a = int(round(t * b))
        for aa in (a - 1, a, a + 1):
            if 0 < aa <= b:
                v = np.float32(aa) / np.float32(b)
                if v < f and (lo is None or v > lo[0]):
                    lo = (v, (aa, b))
                if v > f and (hi is None or v < hi[0]):
                    hi = (v, (aa, b))
    return [lo[1], hi[1]]


def _pair(h, w, c, box_ab, mask_ab, score=0.9):
    """One detection and one GT of class c: box IoU = a/b (full-height boxes, x in pixels of a 64-wide image: exact fp32
    operands), mask IoU = a'/b' (two pixel strips of the flat mask)."""
    a, b = box_ab
    d = a + (b - a) // 2
    g = b - d + a
    det_box = [0, 0, d, h]
    gt_box = [(d - a) / w, 0.0, (d - a + g) / w, 1.0, c]
    ma, mb = mask_ab
    md = ma + (mb - ma) // 2
    mg = mb - md + ma
    return det_box, _strip(h, w, 0, md), gt_box, _strip(h, w, md - ma, md - ma + mg)


def case_thresholds():
    h, w = 48, 64
    imgs = []
    fr = list(FRACTIONS)
    for t in [x / 100 for x in range(50, 100, 5)]:
        fr += _near_fp32(t, 64)
    mfr = list(FRACTIONS)
    for t in [x / 100 for x in range(50, 100, 5)]:
        mfr += _near_fp32(t, h * w)
    for q, (bab, mab) in enumerate(zip(fr, (mfr * 2)[:len(fr)])):
        c = q % 7
        db, dm, gb, gm = _pair(h, w, c, bab, mab, 0.9)
        imgs.append(_image(h, w, [c], [0.9 - 0.01 * q], [db], [dm], [gb], [gm], 0))
    # two GT with the same IoU against one detection: the first j wins; a second detection of lower score takes the other
    db, dm, gb, gm = _pair(h, w, 3, (3, 4), (3, 4))
    imgs.append(_image(h, w, [3, 3], [0.8, 0.7], [db, db], [dm, dm], [gb, gb], [gm, gm], 0))
    # greedy: the higher-scored detection takes the better GT even though the other detection overlaps it more
    db1, dm1, gb1, gm1 = _pair(h, w, 5, (4, 5), (4, 5))
    _, _, gb2, gm2 = _pair(h, w, 5, (3, 5), (3, 5))
    imgs.append(_image(h, w, [5, 5], [0.6, 0.95], [db1, db1], [dm1, dm1], [gb2, gb1], [gm2, gm1], 0))
    return imgs


def case_crowd():
    h, w = 48, 64
    imgs = []
    for q, (a, b) in enumerate(FRACTIONS + [(5, 9), (2, 3), (7, 8)]):
        c = q % 4
        d = b                                                       # crowd IoU = inter / area(det) = a / b
        det_box, det_mask = [0, 0, d, h], _strip(h, w, 0, d * 10)
        crowd_box = [(d - a) / w, 0.0, (d - a + 20) / w, 1.0, c]
        crowd_mask = _strip(h, w, (d - a) * 10, (d - a) * 10 + 400)
        # a real GT of the class at IoU 0.6 against a second detection; the first detection only sees the crowd
        db, dm, gb, gm = _pair(h, w, c, (3, 5), (3, 5))
        other = [(d - a) / w, 0.0, (d - a + 20) / w, 1.0, (c + 1) % 4]
        imgs.append(_image(h, w, [c, c], [0.7, 0.8], [det_box, db], [det_mask, dm],
                           [gb, other, crowd_box], [gm, crowd_mask, crowd_mask], 2))
    # crowd of class -1 (what COCODetection gives crowds): matches nothing
    db, dm, gb, gm = _pair(h, w, 1, (1, 2), (1, 2))
    imgs.append(_image(h, w, [1, 1], [0.5, 0.4], [db, db], [dm, dm], [gb, gb[:4] + [-1]], [gm, gm], 1))
    # a detection matched by real GT at low thresholds and by a crowd at high ones
    db, dm, gb, gm = _pair(h, w, 2, (11, 20), (11, 20))
    crowd = [0.0, 0.0, 1.0, 1.0, 2]
    imgs.append(_image(h, w, [2], [0.65], [db], [dm], [gb, crowd], [gm, np.ones((h, w), np.uint8)], 1))
    return imgs


def random_images(rng, n_images, h, w, n_classes=6, max_det=10, max_gt=6, max_crowd=2, score_grid=20, p_empty=0.1,
                  p_two=0.3, p_nodet=0.05, p_allcrowd=0.05, planted=True):
    """Random images with the features the semantics hinge on: coarse score grids (ties inside and across images, 0, -0.0 and
    negative scores under two-score rescoring), empty masks and zero-area boxes (NaN IoUs), GT copied from detections and moved
    (IoUs near the thresholds), all-crowd images, images without detections."""
    imgs = []
    for _ in range(n_images):
        N = 0 if rng.random() < p_nodet else int(rng.integers(1, max_det + 1))
        n_crowd = int(rng.integers(0, max_crowd + 1))
        G = 0 if rng.random() < p_allcrowd else int(rng.integers(0, max_gt + 1))

        def rand_box():
            x0, x1 = sorted(rng.integers(0, w + 1, 2))
            y0, y1 = sorted(rng.integers(0, h + 1, 2))
            if rng.random() < p_empty:
                x1 = x0
            return [int(x0), int(y0), int(x1), int(y1)]

        def rand_mask(box):
            m = np.zeros((h, w), np.uint8)
            if rng.random() >= p_empty:
                x0, y0, x1, y1 = box
                m[y0:max(y1, y0 + 1), x0:max(x1, x0 + 1)] = 1
                m &= (rng.random((h, w)) < 0.9).astype(np.uint8)
            return m

        cls = rng.integers(0, n_classes, N)
        sc = rng.integers(0, score_grid + 1, N).astype(np.float32) / np.float32(score_grid)
        boxes = [rand_box() for _ in range(N)]
        masks = [rand_mask(b) for b in boxes]
        gt, gtm = [], []
        for j in range(G + n_crowd):
            if planted and N and rng.random() < 0.6:                    # a detection's geometry, moved by a pixel or two
                i = int(rng.integers(0, N))
                x0, y0, x1, y1 = boxes[i]
                dx = int(rng.integers(-2, 3))
                b = [min(max(x0 + dx, 0), w), y0, min(max(x1 + dx, 0), w), y1]
                m = np.roll(masks[i], dx, axis=1)
                c = int(cls[i]) if rng.random() < 0.8 else int(rng.integers(0, n_classes))
            else:
                b = rand_box()
                m = rand_mask(b)
                c = int(rng.integers(0, n_classes))
            if j >= G and rng.random() < 0.2:
                c = -1
            gt.append([b[0] / w, b[1] / h, b[2] / w, b[3] / h, c])
            gtm.append(m)
        sc2 = None
        if N and rng.random() < p_two:
            sc2 = (sc * (rng.integers(-4, 21, N).astype(np.float32) / np.float32(20))).astype(np.float32)
            sc2[rng.random(N) < 0.2] = np.float32(-0.0)
        imgs.append(_image(h, w, cls, sc, boxes, masks, gt, gtm, n_crowd, sc2))
    return imgs


def case_edges():
    rng = np.random.default_rng(11)
    h, w = 12, 16
    imgs = random_images(rng, 30, h, w, p_empty=0.35, p_nodet=0.2, p_allcrowd=0.3)
    z = np.zeros((h, w), np.uint8)
    full = np.ones((h, w), np.uint8)
    # empty mask and zero-area box against an empty GT mask / zero-area GT box and against a crowd: 0 / 0
    imgs.append(_image(h, w, [0, 0], [0.9, 0.8], [[3, 3, 3, 9], [0, 0, 16, 12]], [z, full],
                       [[3 / w, 3 / h, 3 / w, 9 / h, 0], [0, 0, 1, 1, 0]], [z, z], 1))
    # all GT are crowd (G = 0), and a detection-only class (7)
    imgs.append(_image(h, w, [1, 7], [0.5, 0.4], [[0, 0, 8, 8], [0, 0, 8, 8]], [full, full], [[0, 0, 0.5, 0.5, 1]], [full], 1))
    # no detections: GT of class 8 (seen nowhere else) and of class 1 are not counted
    imgs.append(_image(h, w, [], [], np.zeros((0, 4)), np.zeros((0, h, w)), [[0, 0, 1, 1, 8], [0, 0, 1, 1, 1]], [full, full], 0))
    # a GT-only class (9), no crowd
    imgs.append(_image(h, w, [1], [0.3], [[0, 0, 16, 12]], [full], [[0, 0, 1, 1, 9], [0, 0, 1, 1, 1]], [full, full], 0))
    # no GT at all
    imgs.append(_image(h, w, [2], [0.2], [[0, 0, 4, 4]], [full], np.zeros((0, 5)), np.zeros((0, h, w)), 0))
    return imgs


def case_ties():
    rng = np.random.default_rng(23)
    return random_images(rng, 40, 12, 16, n_classes=3, max_det=12, score_grid=4, p_two=0.5)


def case_many():
    rng = np.random.default_rng(5)
    return random_images(rng, 300, 12, 16, n_classes=6, max_det=8, max_gt=5, score_grid=40, p_empty=0.05)


def build_cases():
    return {'thresholds': case_thresholds(), 'crowd': case_crowd(), 'edges': case_edges(), 'ties': case_ties(), 'many': case_many()}


def pack_case(name, imgs):
    """Images -> flat arrays (detections, GT, packed masks) + meta; images_from_arrays is the inverse."""
    out = {}
    meta = {'h': imgs[0]['h'], 'w': imgs[0]['w'], 'num_classes': NUM_CLASSES,
            'images': [{'N': len(im['cls']), 'n_gt': int(im['gt'].shape[0]), 'num_crowd': im['num_crowd'],
                        'two': im['score2'] is not None} for im in imgs]}
    cat = lambda k, shape: np.concatenate([im[k].reshape(shape) for im in imgs])
    out[name + '_cls'] = cat('cls', (-1,))
    out[name + '_score'] = cat('score', (-1,))
    out[name + '_score2'] = np.concatenate([im['score2'] for im in imgs if im['score2'] is not None] or [np.zeros(0, np.float32)])
    out[name + '_box'] = cat('box', (-1, 4))
    out[name + '_maskbits'] = np.packbits(cat('masks', (-1,)))
    out[name + '_gt'] = cat('gt', (-1, 5))
    out[name + '_gtmaskbits'] = np.packbits(cat('gt_masks', (-1,)))
    out[name + '_meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return out


def images_from_arrays(arrays, name):
    meta = json.loads(bytes(arrays[name + '_meta']).decode())
    h, w = meta['h'], meta['w']
    hw = h * w
    n_det = sum(m['N'] for m in meta['images'])
    n_gt = sum(m['n_gt'] for m in meta['images'])
    masks = np.unpackbits(arrays[name + '_maskbits'])[:n_det * hw].reshape(n_det, h, w)
    gtm = np.unpackbits(arrays[name + '_gtmaskbits'])[:n_gt * hw].reshape(n_gt, h, w)
    imgs, d, g, s2 = [], 0, 0, 0
    for m in meta['images']:
        N, n = m['N'], m['n_gt']
        score2 = None
        if m['two']:
            score2 = arrays[name + '_score2'][s2:s2 + N]
            s2 += N
        imgs.append(_image(h, w, arrays[name + '_cls'][d:d + N], arrays[name + '_score'][d:d + N], arrays[name + '_box'][d:d + N],
                           masks[d:d + N], arrays[name + '_gt'][g:g + n], gtm[g:g + n], m['num_crowd'], score2))
        d += N
        g += n
    return meta, imgs


def post_of(im):
    """What the reference's postprocess would have returned for this image (classes, scores, boxes, masks [N,h,w] float)."""
    classes = torch.from_numpy(im['cls'])
    scores = torch.from_numpy(im['score'])
    if im['score2'] is not None:
        scores = [scores, torch.from_numpy(im['score2'])]
    return classes, scores, torch.from_numpy(im['box']), torch.from_numpy(im['masks'].astype(np.float32))


def record(name, ap_data, calc_map, round_off):
    out = {}
    C = NUM_CLASSES
    ap = np.zeros((2, 10, C))
    ngt = np.zeros((2, 10, C), np.int64)
    cnt = np.zeros((2, 10, C), np.int64)
    sc, tp = [], []
    for t, typ in enumerate(('box', 'mask')):
        for k in range(10):
            for c in range(C):
                o = ap_data[typ][k][c]
                pts = list(o.data_points)                   # insertion order (get_ap sorts in place)
                cnt[t, k, c] = len(pts)
                ngt[t, k, c] = o.num_gt_positives
                sc += [float(p[0]) for p in pts]
                tp += [bool(p[1]) for p in pts]
                ap[t, k, c] = np.nan if o.is_empty() else o.get_ap()
    out[name + '_ap'] = ap
    out[name + '_ngt'] = ngt
    out[name + '_dp_count'] = cnt
    out[name + '_dp_score'] = np.array(sc, np.float64)
    out[name + '_dp_tp'] = np.array(tp, bool)
    with round_off():
        maps = calc_map(ap_data)
    keys = list(maps['box'].keys())
    out[name + '_map_keys'] = np.array([str(k) for k in keys])
    for typ in ('box', 'mask'):
        out['%s_map_%s' % (name, typ)] = np.array([maps[typ][k] for k in keys], np.float64)
    maps_r = calc_map(ap_data)
    for typ in ('box', 'mask'):
        out['%s_map_%s_rounded' % (name, typ)] = np.array([maps_r[typ][k] for k in keys], np.float64)
    return out


def main():
    import contextlib
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    from make_golden import _shim_reference
    _shim_reference()                                               # also puts the reference checkout on sys.path
    torch.Tensor.cuda = lambda self, *a, **k: self                 # eval.py:416-417 hard-call .cuda()
    from data import set_cfg
    import eval as E
    E.parse_args(['--no_bar', '--cuda=False'])
    set_cfg('yolact_base_config')
    E.print_maps = lambda all_maps: None
    ref_mask_iou = E.mask_iou

    def mask_iou(masks_a, masks_b, iscrowd=False):
        # box_utils.py:106-107 `.view(0, -1)` raises on an empty operand in this torch (G = 0: every GT is a crowd); the
        # reference's expression is then the empty [A, 0] matrix
        if masks_b.size(0) == 0:
            return torch.zeros(masks_a.size(0), 0)
        return ref_mask_iou(masks_a, masks_b, iscrowd)
    E.mask_iou = mask_iou

    @contextlib.contextmanager
    def round_off():
        E.round = lambda u, n: u                                    # eval.py:1030 rounds through the builtin
        try:
            yield
        finally:
            del E.round

    out = {}
    for name, imgs in build_cases().items():
        out.update(pack_case(name, imgs))
        _, imgs = images_from_arrays(out, name)                     # score exactly what the file holds
        ap_data = {'box': [[E.APDataObject() for _ in range(NUM_CLASSES)] for _ in E.iou_thresholds],
                   'mask': [[E.APDataObject() for _ in range(NUM_CLASSES)] for _ in E.iou_thresholds]}
        for b, im in enumerate(imgs):
            post = post_of(im)
            E.postprocess = lambda dets, w_, h_, **kw: post
            E.prep_metrics(ap_data, None, None, im['gt'], im['gt_masks'].astype(np.float32), im['h'], im['w'], im['num_crowd'], b, None)
        rec = record(name, ap_data, E.calc_map, round_off)
        out.update(rec)
        print('%-10s %3d images  %6d data points  box mAP %.4f  mask mAP %.4f' % (
            name, len(imgs), rec[name + '_dp_tp'].size, rec[name + '_map_box'][0], rec[name + '_map_mask'][0]))
    path = os.path.join(ROOT, 'tests', 'golden', 'ap_eval.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
