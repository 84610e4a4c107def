"""Generate tests/golden/traditional_nms.npz by EXECUTING THE REFERENCE ITSELF with use_fast_nms = False (build container only).

    python tools/make_golden_traditional_nms.py            # needs the reference checkout; writes tests/golden/traditional_nms.npz

The reference model runs on CPU exactly as oracle/make_golden.run_case runs it (same shims, same CASES rows, same synthetic parameters
and images), but with Detect.use_fast_nms = False, so that its own Detect.detect / traditional_nms glue (detection.py:80-108,182-228)
produces the detections.  Its Cython NMS (utils/cython_nms.pyx) cannot be compiled with Cython 3 + numpy 2 (np.int_t), so
`greedy_nms` below — an fp32 numpy statement of the same greedy algorithm — is registered as `utils.cython_nms` first.

Recorded per image: box, coef, class, score and prior index of every detection, and whether the image is DECIDABLE, i.e. its result
does not hinge on a rounding: every overlap the greedy pass compared is at least 1e-5 from nms_thresh, no two candidates of a class
have tied scores, and the cut at max_num_detections does not fall inside a tie of scores.  Per-class candidate counts K are printed
(and stored): K > 4096 is the device's global-memory path (csrc/detect_greedy.hip KLDS).
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IOU_MARGIN = 1e-5
KLDS = 4096

# (name, CASES row of oracle/make_golden.py, overrides of the reference's Detect)
TN_CASES = [
    ('r50_dense', 'r50_dense', {}),
    ('r50_sparse', 'r50_sparse', {}),
    ('r50_few', 'r50_few', {}),
    ('im700', 'im700', {}),
    ('plus_r50', 'plus_r50', {}),
    ('r50_cc', 'r50_cc', {'cross_class': True}),
    # every prior is a candidate of every class (conf_thresh below 1/81): K = P, the device's large-K path
    ('r50_largek', 'r50_sparse', {'conf_thresh': 0.005}),
]


def greedy_nms(dets, thresh, log=None):
    """Greedy NMS of cython_nms.pyx's contract: dets [n,5] fp32 (x1, y1, x2, y2, score) in pixels -> indices of the kept rows,
    ascending.  Visits rows by descending score (ties: lower row first), a kept row suppresses every later unsuppressed row whose
    overlap inter / (area_i + area_j - inter) is >= thresh, with areas and sides counted "+1".  All arithmetic in fp32."""
    dets = np.ascontiguousarray(dets, dtype=np.float32)
    x1, y1, x2, y2, sc = (dets[:, k].copy() for k in range(5))
    one, zero, th = np.float32(1), np.float32(0), np.float32(thresh)
    areas = (x2 - x1 + one) * (y2 - y1 + one)
    order = np.argsort(-sc, kind='stable')
    n = dets.shape[0]
    suppressed = np.zeros(n, dtype=bool)
    margin = np.inf
    for _i in range(n):
        i = order[_i]
        if suppressed[i]:
            continue
        rest = order[_i + 1:]
        rest = rest[~suppressed[rest]]
        if rest.size == 0:
            continue
        xx1 = np.maximum(x1[i], x1[rest])
        yy1 = np.maximum(y1[i], y1[rest])
        xx2 = np.minimum(x2[i], x2[rest])
        yy2 = np.minimum(y2[i], y2[rest])
        w = np.maximum(zero, xx2 - xx1 + one)
        h = np.maximum(zero, yy2 - yy1 + one)
        inter = w * h
        ovr = inter / (areas[i] + areas[rest] - inter)
        assert ovr.dtype == np.float32
        suppressed[rest[ovr >= th]] = True
        margin = min(margin, float(np.abs(ovr.astype(np.float64) - float(th)).min()))
    keep = np.where(~suppressed)[0]
    if log is not None:
        log.append(dict(n=n, margin=margin, tied=bool(np.unique(sc).size != n), keep=keep))
    return keep


def run_case(tn_name, row, over, log):
    from yolact_amd.utils.synth import synth_state_dict, synth_images
    name, config, B, size, seed, gain = row[:6]
    extra = row[7] if len(row) > 7 else {}
    from data import cfg, set_cfg
    set_cfg(config)
    cfg.mask_proto_debug = False
    from yolact import Yolact
    torch.manual_seed(0)
    net = Yolact()
    net.eval()
    net.detect.use_fast_nms = False
    net.detect.use_cross_class_nms = bool(over.get('cross_class', extra.get('cross_class', False)))
    if 'conf_thresh' in over:
        net.detect.conf_thresh = float(over['conf_thresh'])
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(synth_state_dict(shapes, seed=seed, conf_gain=gain, bg_bias=extra.get('bg_bias', 0.0)))
    x = synth_images(B, size, size, seed=1000 + seed)
    det = net.detect
    thr = float(det.conf_thresh)
    ctx = {}
    real_detect = det.detect

    def detect_obs(batch_idx, conf_preds, decoded_boxes, mask_data, inst_data):
        # observation only: which priors / classes the reference's own glue will hand to the NMS routine, in call order
        cur = conf_preds[batch_idx, 1:, :]
        kidx = torch.nonzero(cur.max(0)[0] > thr).squeeze(1)
        sc = cur[:, kidx]
        ctx[batch_idx] = dict(kidx=kidx, scores=sc, mask=mask_data[batch_idx], calls=[])
        log['cur'] = ctx[batch_idx]['calls']
        return real_detect(batch_idx, conf_preds, decoded_boxes, mask_data, inst_data)
    det.detect = detect_obs
    sys.modules['utils.cython_nms'].nms = lambda dets, th: greedy_nms(dets, th, log['cur'])
    with torch.no_grad():
        dets = net(x)
    del det.detect
    arrays, meta_imgs = {}, []
    max_det = int(cfg.max_num_detections)
    for b, d in enumerate(dets):
        c = ctx[b]
        sc = c['scores']                                      # [C-1, K_kept]
        ncand = (sc > thr).sum(1)
        Ks = [int(v) for v in ncand]
        classes_called = [k for k in range(sc.shape[0]) if Ks[k] > 0]
        assert len(classes_called) == len(c['calls']), (len(classes_called), len(c['calls']))
        r = d['detection']
        info = dict(K_max=max(Ks) if Ks else 0, K_sum=sum(Ks), n_classes=len(classes_called),
                    n_large=sum(1 for k in Ks if k > KLDS))
        if r is None:
            info.update(n=0, decidable=True, iou_margin=None, tied=False, cut_tied=False)
            meta_imgs.append(info)
            continue
        n = int(r['score'].shape[0])
        # prior index of every returned row: its class, score and coefficient row identify it among the candidates of the class
        prior = np.empty(n, dtype=np.int64)
        for i in range(n):
            k = int(r['class'][i])
            cols = torch.nonzero(sc[k] == r['score'][i]).squeeze(1)
            cols = [int(j) for j in cols if torch.equal(c['mask'][c['kidx'][j]], r['mask'][i])]
            assert len(cols) == 1, (tn_name, b, i, cols)
            prior[i] = int(c['kidx'][cols[0]])
        iou_margin = min(cl['margin'] for cl in c['calls'])
        tied = any(cl['tied'] for cl in c['calls'])
        # does the cut at max_det fall inside a tie of the survivors' scores?
        surv = np.sort(np.asarray(_survivor_scores(c, classes_called, thr), dtype=np.float32))[::-1]
        cut_tied = bool(surv.size > max_det and surv[max_det - 1] == surv[max_det])
        info.update(n=n, iou_margin=iou_margin, tied=tied, cut_tied=bool(cut_tied),
                    decidable=bool(iou_margin >= IOU_MARGIN and not tied and not cut_tied))
        meta_imgs.append(info)
        arrays['%s_%d_box' % (tn_name, b)] = r['box'].numpy().astype(np.float32)
        arrays['%s_%d_coef' % (tn_name, b)] = r['mask'].numpy().astype(np.float32)
        arrays['%s_%d_class' % (tn_name, b)] = r['class'].numpy().astype(np.int64)
        arrays['%s_%d_score' % (tn_name, b)] = r['score'].numpy().astype(np.float32)
        arrays['%s_%d_prior' % (tn_name, b)] = prior
    meta = dict(name=tn_name, source=name, config=config, B=B, size=size, seed=seed, conf_gain=gain,
                bg_bias=extra.get('bg_bias', 0.0), cross_class=bool(net.detect.use_cross_class_nms), conf_thresh=thr,
                nms_thresh=float(det.nms_thresh), max_det=max_det, max_size=int(cfg.max_size), images=meta_imgs)
    for b, im in enumerate(meta_imgs):
        print('%-11s img %d: n=%-3d decidable=%-5s K per class max %-5d sum %-7d classes %-2d large-K classes %-2d iou margin %s'
              % (tn_name, b, im['n'], im['decidable'], im['K_max'], im['K_sum'], im['n_classes'], im['n_large'], im['iou_margin']))
    return meta, arrays


def _survivor_scores(c, classes_called, thr):
    """Scores of every per-class survivor of one image (the list the reference sorts and cuts at max_det)."""
    out = []
    for k, cl in zip(classes_called, c['calls']):
        out.extend(c['scores'][k][c['scores'][k] > thr][torch.as_tensor(cl['keep'])].tolist())
    return out


def main():
    from oracle.make_golden import CASES, _shim_reference
    _shim_reference(with_dcn_oracle=True)
    mod = types.ModuleType('utils.cython_nms')
    mod.nms = greedy_nms
    sys.modules['utils.cython_nms'] = mod
    rows = {c[0]: c for c in CASES}
    only = sys.argv[1:]
    metas, arrays = [], {}
    for tn_name, src, over in TN_CASES:
        if only and tn_name not in only:
            continue
        log = {}
        meta, arr = run_case(tn_name, rows[src], over, log)
        metas.append(meta)
        arrays.update(arr)
    arrays['meta'] = np.frombuffer(json.dumps(dict(cases=metas, iou_margin=IOU_MARGIN, torch=torch.__version__)).encode(),
                                   dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'traditional_nms.npz')
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
