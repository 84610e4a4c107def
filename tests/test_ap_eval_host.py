"""On-device COCO mAP evaluation, host side: the golden fixture (the reference's own evaluator), its test-side restatement, the
host parts of yolact_amd.evaluation (calc_map from an AP array, GT box scaling) and the C ABI entries' argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import ap_eval_ref as R

CASES = ['thresholds', 'crowd', 'edges', 'ties', 'many']


def _maps_array(maps):
    return (np.array(list(maps['box'].values()), np.float64), np.array(list(maps['mask'].values()), np.float64))


def test_golden_holds_every_case_and_edge():
    z = R.load()
    assert R.generator().CASE_NAMES == CASES
    for name in CASES:
        meta, imgs = R.case(name)
        assert len(imgs) == len(meta['images']) and meta['num_classes'] == 80
        assert list(z[name + '_map_keys']) == ['all'] + [str(x) for x in range(50, 100, 5)]
    _, many = R.case('many')
    assert len(many) >= 300
    _, edges = R.case('edges')
    assert any(len(im['cls']) == 0 and im['gt'].shape[0] > 0 for im in edges)                     # early return
    assert any(im['gt'].shape[0] > 0 and im['gt'].shape[0] == im['num_crowd'] for im in edges)   # G = 0
    assert any(im['num_crowd'] == 0 and im['gt'].shape[0] > 0 for im in edges)                   # Gc = 0
    _, ties = R.case('ties')
    sc2 = np.concatenate([im['score2'] for im in ties if im['score2'] is not None])
    assert (sc2 < 0).any() and np.signbit(sc2[sc2 == 0]).any() and (sc2 == 0).any()
    _, crowd = R.case('crowd')
    assert any((im['gt'][-im['num_crowd']:, 4] == -1).any() for im in crowd if im['num_crowd'])


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_reference(name):
    z = R.load()
    meta, imgs = R.case(name)
    ap_data = R.run(imgs, meta['num_classes'])
    for t, typ in enumerate(('box', 'mask')):
        for k in range(10):
            for c in range(meta['num_classes']):
                o = ap_data[typ][k][c]
                assert o.num_gt_positives == z[name + '_ngt'][t, k, c]
                assert o.data_points == R.golden_points(name, t, k, c), (typ, k, c)
    ap = R.ap_array(ap_data)
    assert np.array_equal(ap, z[name + '_ap'], equal_nan=True)
    box, mask = _maps_array(R.calc_map(ap_data))
    assert np.array_equal(box, z[name + '_map_box']) and np.array_equal(mask, z[name + '_map_mask'])
    box, mask = _maps_array(R.calc_map(ap_data, rounded=True))
    assert np.array_equal(box, z[name + '_map_box_rounded']) and np.array_equal(mask, z[name + '_map_mask_rounded'])


@pytest.mark.parametrize('name', CASES)
def test_calc_map_from_ap_objects_is_bit_exact(name):
    from yolact_amd.evaluation import calc_map_from_ap
    z = R.load()
    maps = calc_map_from_ap(z[name + '_ap'], rounded=False)
    assert list(maps['box'].keys()) == ['all'] + list(range(50, 100, 5))
    box, mask = _maps_array(maps)
    assert np.array_equal(box, z[name + '_map_box']) and np.array_equal(mask, z[name + '_map_mask'])
    box, mask = _maps_array(calc_map_from_ap(z[name + '_ap']))
    assert np.array_equal(box, z[name + '_map_box_rounded']) and np.array_equal(mask, z[name + '_map_mask_rounded'])


def test_calc_map_empty_and_gt_only_classes():
    from yolact_amd.evaluation import calc_map_from_ap
    ap = np.full((2, 10, 5), np.nan)
    maps = calc_map_from_ap(ap, rounded=False)
    assert all(v == 0 for v in maps['box'].values())
    ap[:, :, 1] = 0.0                  # a class with only GT (or only detections): AP 0, counted in the mean
    ap[:, :, 3] = 0.5
    maps = calc_map_from_ap(ap, rounded=False)
    assert maps['mask'][50] == 25.0 and maps['mask']['all'] == 25.0


def test_gt_box_scaling_is_the_reference_float32_expression():
    from yolact_amd.evaluation import gt_boxes_px
    rng = np.random.default_rng(0)
    gt = np.concatenate([rng.random((200, 4)), rng.integers(0, 80, (200, 1))], axis=1)
    for w, h in ((550, 550), (641, 427), (64, 48), (1, 3)):
        ref = torch.Tensor(gt[:, :4])
        ref[:, [0, 2]] *= w
        ref[:, [1, 3]] *= h
        assert np.array_equal(gt_boxes_px(gt, w, h), ref.numpy())


def test_cabi_ap_entries():
    from yolact_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, 'ymi_ap_match_f32') and hasattr(lib, 'ymi_ap_finalize_f64')
    assert L.ABI_VERSION == 9 and L.lib().ymi_abi_version() == 9
    assert ctypes.sizeof(L.ApMatchDesc) == 136 and ctypes.sizeof(L.ApFinalizeDesc) == 72
    d = L.ApMatchDesc()
    d.N, d.G, d.Gc, d.num_classes, d.cap = 5, 3, 0, 80, 100
    assert L.lib().ymi_ap_match_f32(None, None) == -3
    assert L.lib().ymi_ap_match_f32(ctypes.byref(d), None) == -3           # null pointers
    d.N = L.AP_MAX_DET + 1
    assert L.lib().ymi_ap_match_f32(ctypes.byref(d), None) == -1
    d.N, d.base = 5, 96                                                    # base + N > cap
    assert L.lib().ymi_ap_match_f32(ctypes.byref(d), None) == -1
    d.N, d.base = 0, 0                                                     # no detections: nothing to do, no launch
    assert L.lib().ymi_ap_match_f32(ctypes.byref(d), None) == 0
    f = L.ApFinalizeDesc()
    f.M, f.cap, f.num_classes = 10, 5, 80
    assert L.lib().ymi_ap_finalize_f64(ctypes.byref(f), None) == -1
    f.cap = 10
    assert L.lib().ymi_ap_finalize_f64(ctypes.byref(f), None) == -3


def test_to_ap_data_export_matches_the_reference_interface():
    from yolact_amd.evaluation import APData
    ref = R.APDataObject()
    mine = APData()
    for s, t in [(0.5, True), (0.7, False), (0.5, False), (-0.0, True), (0.0, False)]:
        ref.push(s, t)
        mine.push(s, t)
    ref.add_gt_positives(3)
    mine.add_gt_positives(3)
    assert mine.get_ap() == ref.get_ap() and mine.is_empty() == ref.is_empty()
