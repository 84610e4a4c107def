"""On-device COCO mAP evaluation (yolact_amd.evaluation, csrc/ap_eval.hip) against the reference's own evaluator.

  * the golden cases of tests/golden/ap_eval.npz (written by executing the reference's prep_metrics / APDataObject / calc_map):
    every get_ap(), every data point, every GT count and the table, exactly;
  * the six tables of tests/golden/map.npz from the stored reference detections;
  * a seeded random run (300+ images, up to 300 GT, crowds, planted ties, one- and two-score images) against tests/ap_eval_ref.py;
  * end to end: Yolact.forward -> APEvaluator.add equals oracle/map_eval on the same postprocess output; add() reads nothing back;
  * evaluate() equals the hand-written pull_item + add loop.
"""
import json
import os

import numpy as np
import pytest
import torch

import ap_eval_ref as R
from helpers import GOLDEN_DIR, case_images, load_golden

DEV = 'cuda:0'
CASES = ['thresholds', 'crowd', 'edges', 'ties', 'many']
MAP_CASES = ['r50_dense', 'r50_sparse', 'r101_base', 'darknet53', 'im700', 'plus_r50']


def _maps_array(maps):
    return (np.array(list(maps['box'].values()), np.float64), np.array(list(maps['mask'].values()), np.float64))


def _add_image(ev, im):
    from yolact_amd.layers.box_utils import mask_bits
    N = len(im['cls'])
    if N == 0:
        ev.add_detections([], [], [], None, im['gt'], im['gt_masks'], im['h'], im['w'], im['num_crowd'])
        return
    cls = torch.from_numpy(im['cls']).to(DEV)
    sc = torch.from_numpy(im['score']).to(DEV)
    scores = sc if im['score2'] is None else [sc, torch.from_numpy(im['score2']).to(DEV)]
    boxes = torch.from_numpy(im['box']).to(DEV)
    bits = mask_bits(torch.from_numpy(im['masks'].astype(np.float32)).to(DEV))
    ev.add_detections(cls, scores, boxes, bits, im['gt'], im['gt_masks'], im['h'], im['w'], im['num_crowd'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_golden_cases_bit_exact(name):
    from yolact_amd.evaluation import APEvaluator
    z = R.load()
    meta, imgs = R.case(name)
    ev = APEvaluator(meta['num_classes'], DEV)
    for im in imgs:
        _add_image(ev, im)
    ap = ev.ap_objects()
    assert np.array_equal(ap, z[name + '_ap'], equal_nan=True), np.argwhere(~((ap == z[name + '_ap']) |
                                                                            (np.isnan(ap) & np.isnan(z[name + '_ap']))))
    data = ev.to_ap_data()
    for t, typ in enumerate(('box', 'mask')):
        for k in range(10):
            for c in range(meta['num_classes']):
                o = data[typ][k][c]
                assert o.num_gt_positives == z[name + '_ngt'][t, k, c]
                assert o.data_points == R.golden_points(name, t, k, c), (typ, k, c)
    box, mask = _maps_array(ev.calc_map(rounded=False))
    assert np.array_equal(box, z[name + '_map_box']) and np.array_equal(mask, z[name + '_map_mask'])
    box, mask = _maps_array(ev.calc_map())
    assert np.array_equal(box, z[name + '_map_box_rounded']) and np.array_equal(mask, z[name + '_map_mask_rounded'])
    ev.reset()
    assert np.isnan(ev.ap_objects()).all()


@pytest.mark.gpu
@pytest.mark.parametrize('name', MAP_CASES)
def test_map_golden_tables_from_reference_detections(name):
    from test_map_parity import _gold, _gt, _ref_post
    from yolact_amd.evaluation import APEvaluator
    from yolact_amd.layers.box_utils import mask_bits
    z = _gold()
    meta, arrays = load_golden(name)
    w, h = meta['post']
    ev = APEvaluator(80, DEV)
    for b, n in enumerate(meta['n']):
        if n == 0:
            continue
        gt, gm = _gt(z, name, b, w, h)
        classes, scores, boxes, masks = _ref_post(arrays, b, w, h)
        scores = [s.to(DEV) for s in scores] if isinstance(scores, list) else scores.to(DEV)
        ev.add_detections(classes.to(DEV), scores, boxes.to(DEV), mask_bits(masks.to(DEV)), gt, gm.astype(np.uint8), h, w, 0)
    box, mask = _maps_array(ev.calc_map())
    assert np.array_equal(box, z[name + '_box']) and np.array_equal(mask, z[name + '_mask'])


@pytest.mark.gpu
def test_random_run_matches_restatement():
    from yolact_amd.evaluation import APEvaluator
    gen = R.generator()
    rng = np.random.default_rng(2024)
    imgs = gen.random_images(rng, 300, 12, 16, n_classes=8, max_det=12, max_gt=8, max_crowd=3, score_grid=10, p_two=0.4)
    imgs += gen.random_images(rng, 4, 12, 16, n_classes=3, max_det=60, max_gt=300, max_crowd=6, score_grid=10, p_nodet=0.0)
    assert max(im['gt'].shape[0] - im['num_crowd'] for im in imgs) >= 150
    ref = R.run(imgs, 80)
    ev = APEvaluator(80, DEV)
    for im in imgs:
        _add_image(ev, im)
    assert np.array_equal(ev.ap_objects(), R.ap_array(ref), equal_nan=True)
    data = ev.to_ap_data()
    for typ in ('box', 'mask'):
        for k in range(10):
            for c in range(80):
                assert data[typ][k][c].data_points == ref[typ][k][c].data_points
                assert data[typ][k][c].num_gt_positives == ref[typ][k][c].num_gt_positives
    assert ev.calc_map(rounded=False) == R.calc_map(ref)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['r50_sparse', 'plus_r50'])
def test_end_to_end_matches_oracle_evaluator(name):
    from gpu_utils import build_net
    from oracle import map_eval as ME
    from test_map_parity import _gold, _gt
    from yolact_amd.evaluation import APEvaluator
    from yolact_amd.layers.output_utils import postprocess
    z = _gold()
    meta, _ = load_golden(name)
    w, h = meta['post']
    net = build_net(meta)
    with torch.no_grad():
        preds = net(case_images(meta).to(DEV))
    ev = APEvaluator(80, DEV)
    ap = ME.new_ap_data(80)
    for b, n in enumerate(meta['n']):
        if n == 0:
            continue
        gt, gm = _gt(z, name, b, w, h)
        ev.add(preds, gt, gm, h, w, 0, batch_idx=b)
        classes, scores, boxes, masks = postprocess(preds, w, h, batch_idx=b)
        scores = [s.cpu() for s in scores] if isinstance(scores, list) else scores.cpu()
        ME.prep_metrics(ap, classes.cpu(), scores, boxes.cpu(), masks.cpu(), gt, gm, h, w)
    mine = ev.calc_map(rounded=False)
    ref = ME.calc_map(ap, 80)
    assert mine == ref, (mine, ref)
    assert ref['box'][50] > 0 and ref['mask'][50] > 0


@pytest.mark.gpu
def test_add_reads_nothing_back():
    from gpu_utils import build_net
    from test_map_parity import _gold, _gt
    from yolact_amd.evaluation import APEvaluator
    z = _gold()
    meta, _ = load_golden('r50_sparse')
    w, h = meta['post']
    net = build_net(meta)
    with torch.no_grad():
        preds = net(case_images(meta).to(DEV))
    ev = APEvaluator(80, DEV)
    ev.add(preds, *_gt(z, 'r50_sparse', 0, w, h), h, w, 0, batch_idx=0)     # warm-up: library load, first allocations
    gts = [_gt(z, 'r50_sparse', b, w, h) for b, n in enumerate(meta['n']) if n]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for b, (gt, gm) in enumerate(gts):
            ev.add(preds, gt, gm, h, w, 0, batch_idx=b)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert np.isfinite(ev.ap_objects()).any()


@pytest.mark.gpu
def test_evaluate_equals_the_hand_written_loop(tmp_path):
    import bench
    from tests import coco_synth
    from yolact_amd.data import COCODetection
    from yolact_amd.evaluation import APEvaluator, evaluate
    from yolact_amd.utils.augmentations import BaseTransform
    info_file = coco_synth.write_dataset(str(tmp_path))
    dev = torch.device('cuda', 0)
    net, _ = bench.build_model(dev, 550)
    ds = COCODetection(str(tmp_path), info_file, transform=BaseTransform())
    got = evaluate(net, ds, batch_size=2)
    ev = APEvaluator(80, dev)
    n_det = 0
    with torch.no_grad():
        for s in range(0, len(ds), 2):
            items = [ds.pull_item(i) for i in range(s, min(s + 2, len(ds)))]
            preds = net(torch.stack([it[0] for it in items]))
            for b, (_, gt, gm, h, w, num_crowd) in enumerate(items):
                ev.add(preds, gt, gm, h, w, num_crowd, batch_idx=b)
                n_det += ev._n
    assert n_det > 0
    assert got == ev.calc_map()
