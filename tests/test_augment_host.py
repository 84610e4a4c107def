"""SSDAugmentation's host half (no GPU): `draw_augmentation` against draws recorded by EXECUTING the reference's own transform
(tests/golden/augment_draws.npz, tools/make_golden_augment.py), the switches, the refusals, the C ABI additions and the numpy
restatement the GPU tests compare the kernels with."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import augment_ref as R
from oracle import coco_dataset as OD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'augment_draws.npz'))


def _cfg(**kw):
    from yolact_amd.config import CONFIGS
    return CONFIGS['yolact_base_config'].copy(kw)


def _case(c):
    a, b = int(GOLD['case_off'][c]), int(GOLD['case_off'][c + 1])
    h, w = (int(v) for v in GOLD['case_hw'][c])
    return h, w, GOLD['case_boxes'][a:b].copy(), {'labels': GOLD['case_labels'][a:b].copy(), 'num_crowds': int(GOLD['case_num_crowds'][c])}


def test_draws_reproduce_every_recorded_run_of_the_reference():
    from yolact_amd.utils.augmentations import draw_augmentation
    cfg = _cfg()
    runs = len(GOLD['run_case'])
    assert runs >= 64 and len(GOLD['case_hw']) >= 4
    for r in range(runs):
        h, w, boxes, labels = _case(int(GOLD['run_case'][r]))
        before = boxes.copy()
        np.random.seed(int(GOLD['run_seed'][r]))
        p, out_boxes, out_labels = draw_augmentation(h, w, boxes, labels, cfg)
        trail = np.random.uniform()
        s, e = int(GOLD['run_off'][r]), int(GOLD['run_off'][r + 1])
        what = (GOLD['case_name'][int(GOLD['run_case'][r])], int(GOLD['run_seed'][r]))
        assert out_boxes.dtype == np.float64 and np.array_equal(out_boxes, GOLD['run_boxes'][s:e]), what
        assert np.array_equal(out_labels['labels'], GOLD['run_labels'][s:e]), what
        assert int(out_labels['num_crowds']) == int(GOLD['run_num_crowds'][r]), what
        assert (p.crop_h, p.crop_w) == tuple(GOLD['run_pre_shape'][r]), what
        assert trail == GOLD['run_trail'][r], what                      # the same number of draws was consumed
        assert np.array_equal(boxes, before)                            # the caller's arrays are left alone
        # the record is consistent with the ground truth it returns
        assert len(p.keep) == e - s and np.array_equal(labels['labels'][p.keep], out_labels['labels'])
        assert 0 <= p.off_x and p.off_x + w <= p.canvas_w and 0 <= p.off_y and p.off_y + h <= p.canvas_h
        assert 0 <= p.crop[0] < p.crop[2] <= p.canvas_w and 0 <= p.crop[1] < p.crop[3] <= p.canvas_h


def test_each_switch_off_consumes_no_draws():
    from yolact_amd.utils.augmentations import draw_augmentation
    h, w, boxes, labels = _case(0)
    off = dict(augment_photometric_distort=False, augment_expand=False, augment_random_sample_crop=False,
               augment_random_mirror=False)
    np.random.seed(5)
    first = np.random.uniform()
    np.random.seed(5)
    p, out_boxes, out_labels = draw_augmentation(h, w, boxes, labels, _cfg(**off))
    assert np.random.uniform() == first                                 # everything off: the stream is untouched
    assert not p.photometric and not p.mirror and p.crop == (0, 0, w, h) and (p.canvas_h, p.canvas_w, p.off_x, p.off_y) == (h, w, 0, 0)
    assert np.allclose(out_boxes, boxes, rtol=1e-14, atol=0) and list(p.keep) == list(range(len(boxes)))

    class Counting:
        """numpy.random with a count of the calls."""
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def f(*a, **kw):
                self.calls.append(name)
                return getattr(np.random, name)(*a, **kw)
            return f

    counts = {}
    for only in off:
        rng = Counting()
        np.random.seed(7)
        draw_augmentation(h, w, boxes, labels, _cfg(**{k: (k == only) for k in off}), rng=rng)
        counts[only] = rng.calls
    assert counts['augment_random_mirror'] == ['randint']
    assert counts['augment_expand'][0] == 'randint' and set(counts['augment_expand'][1:]) <= {'uniform'}
    assert counts['augment_random_sample_crop'][0] == 'choice'
    # brightness flag, order flag, three stage flags at the least; each flag at most one uniform
    ph = counts['augment_photometric_distort']
    assert ph.count('randint') == 5 and ph.count('uniform') <= 4 and 'choice' not in ph


@pytest.mark.parametrize('field', ['augment_random_flip', 'use_gt_bboxes', 'preserve_aspect_ratio'])
def test_unsupported_settings_are_refused_by_name(field):
    from yolact_amd.utils.augmentations import SSDAugmentation, draw_augmentation
    h, w, boxes, labels = _case(0)
    with pytest.raises(NotImplementedError, match=field):
        draw_augmentation(h, w, boxes, labels, _cfg(**{field: True}))
    import yolact_amd
    from yolact_amd.config import active_cfg
    yolact_amd.set_cfg('yolact_base_config')
    cfg = active_cfg()                      # the object the transform reads at call time
    was = getattr(cfg, field)
    setattr(cfg, field, True)
    try:
        with pytest.raises(NotImplementedError, match=field):
            SSDAugmentation()(torch.zeros(h, w, 3, dtype=torch.uint8), np.zeros((len(boxes), h, w), np.uint8), boxes, labels)
    finally:
        setattr(cfg, field, was)


def test_cpu_image_without_a_gpu_is_refused(monkeypatch):
    import yolact_amd
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    from yolact_amd.utils.augmentations import SSDAugmentation
    yolact_amd.set_cfg('yolact_base_config')
    h, w, boxes, labels = _case(0)
    aug = SSDAugmentation()
    with pytest.raises(RuntimeError, match='GPU'):
        aug(np.zeros((h, w, 3), np.uint8), np.zeros((len(boxes), h, w), np.uint8), boxes, labels)
    with pytest.raises(RuntimeError, match='GPU'):
        aug.batch([(torch.zeros(h, w, 3), np.zeros((len(boxes), h, w), np.uint8), boxes, labels)])


def test_config_has_the_reference_defaults():
    from yolact_amd.config import CONFIGS
    for cfg in CONFIGS.values():
        assert cfg.augment_photometric_distort and cfg.augment_expand and cfg.augment_random_sample_crop and cfg.augment_random_mirror
        assert not cfg.augment_random_flip and not cfg.augment_random_rot90 and not cfg.use_gt_bboxes and not cfg.preserve_aspect_ratio
        assert cfg.discard_box_width == 4 / 550 and cfg.discard_box_height == 4 / 550


def test_abi_header_and_binding_agree():
    from yolact_amd import _lib as L
    hdr = open(os.path.join(ROOT, 'include', 'yolact_amd.h')).read()
    assert L.WS_AUGMENT == 27 and 'YMI_WS_AUGMENT = 27' in hdr and L.ABI_VERSION == 9 and '#define YMI_ABI_VERSION 9' in hdr
    assert re.search(r'int ymi_ssd_augment_f32\(const ymi_augment_desc \*d, void \*stream\);', hdr)
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    assert bound['ymi_ssd_augment_f32'] == (C.c_int, [C.POINTER(L.AugmentDesc), C.c_void_p])
    flags = dict(re.findall(r'YMI_AUG_([A-Z0-9_]+) = (\d+)', hdr))
    assert {k: int(v) for k, v in flags.items()} == {k[4:]: getattr(L, k) for k in dir(L) if k.startswith('AUG_')}
    assert C.sizeof(L.AugmentRec) == 2 * 8 + 20 * 4 and C.sizeof(L.AugmentDesc) == 5 * 8 + 8 + 6 * 4 + 6 * 4
    lib = L.lib()
    assert lib.ymi_abi_version() == 9
    d = L.AugmentDesc(B=3, n_masks=5)
    assert lib.ymi_workspace_bytes(L.WS_AUGMENT, C.byref(d)) == 3 * 96 + 48 + 3 * 16
    assert lib.ymi_workspace_bytes(L.WS_AUGMENT, C.byref(L.AugmentDesc(B=1, n_masks=0))) == 96 + 16
    assert lib.ymi_workspace_bytes(L.WS_AUGMENT, C.byref(L.AugmentDesc(B=0))) == -1
    assert lib.ymi_workspace_bytes(L.WS_AUGMENT, None) == -3
    # validation happens before anything touches a device: these return without a GPU
    assert lib.ymi_ssd_augment_f32(None, None) == -3
    assert lib.ymi_ssd_augment_f32(C.byref(L.AugmentDesc(B=1, S=8)), None) == -3


def test_detection_collate_is_the_references():
    from yolact_amd.data import detection_collate
    items = [(torch.zeros(3, 4, 4), (np.array([[0.1, 0.2, 0.3, 0.4, 5.0]]), np.ones((1, 4, 4), np.uint8), 0)),
             (torch.ones(3, 4, 4), (np.zeros((2, 5)), torch.zeros(2, 4, 4), 1))]
    imgs, (targets, masks, num_crowds) = detection_collate(items)
    assert len(imgs) == 2 and imgs[1] is items[1][0] and num_crowds == [0, 1]
    assert [t.dtype for t in targets + masks] == [torch.float32] * 4
    assert tuple(targets[0].shape) == (1, 5) and tuple(masks[1].shape) == (2, 4, 4) and masks[0].sum().item() == 16


def test_shim_module_reexports():
    import importlib.util
    spec = importlib.util.spec_from_file_location('shim_utils_augmentations', os.path.join(ROOT, 'shim', 'utils', 'augmentations.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    import yolact_amd.utils.augmentations as A
    assert m.SSDAugmentation is A.SSDAugmentation and m.BaseTransform is A.BaseTransform and m.draw_augmentation is A.draw_augmentation


# ---- the restatement itself --------------------------------------------------------------------------------------------------

def test_restated_float_resize_is_the_oracles():
    rng = np.random.RandomState(3)
    for (h, w), S in (((37, 53), 24), ((64, 48), 40), ((5, 7), 24)):
        img = (rng.rand(h, w, 3) * 255).astype(np.float32)
        assert np.array_equal(R.resize_linear(img, S, S, np.float32), OD.cv2_resize_linear_f32(img, S, S))


def test_restated_hsv_round_trip_and_known_colours():
    f = np.float64
    px = np.array([[[0, 0, 255], [0, 255, 0], [255, 0, 0], [0, 255, 255], [128, 128, 128], [-32, -32, -32]]], dtype=f)   # BGR
    hsv = R.bgr_to_hsv(px, f)
    assert np.allclose(hsv[0, :4, 0], [0, 120, 240, 60]) and np.allclose(hsv[0, :4, 1], 1) and np.allclose(hsv[0, :, 2], [255] * 4 + [128, -32])
    assert hsv[0, 4, 1] == 0 and hsv[0, 5, 1] == 0 and hsv[0, 5, 2] == -32        # grey: no saturation; a negative V stays
    rng = np.random.RandomState(0)
    img = rng.rand(16, 16, 3) * 300 + 1            # (a negative V does not survive the round trip: S divides by |V|)
    assert np.abs(R.hsv_to_bgr(R.bgr_to_hsv(img, f), f) - img).max() < 1e-6        # FLT_EPSILON in S's denominator
    img32 = img.astype(np.float32)
    back = R.hsv_to_bgr(R.bgr_to_hsv(img32, np.float32), np.float32)
    assert back.dtype == np.float32 and np.abs(back - img32).max() < 1e-3
    # hue + 360 is the same colour; the wrap keeps H in [0, 360]
    from yolact_amd.utils.augmentations import AugmentParams
    p = AugmentParams(height=16, width=16, photometric=True, hue=18.0)
    q = AugmentParams(height=16, width=16, photometric=True, hue=-18.0)
    a = R.photometric(R.photometric(img, p, f), q, f)
    assert np.abs(a - img).max() < 1e-6


def test_restated_mask_rule():
    m = np.zeros((6, 8), np.uint8)
    m[2:5, 3:7] = 1
    assert np.array_equal(R.resize_mask_u8(m, 8, 6), m)                                   # same size: every fraction is 0
    up = R.resize_mask_u8(m, 16, 12)
    assert set(np.unique(up)) <= {0, 1} and up[6, 9] == 1 and up[0, 0] == 0
    # a 1 x 2 mask [0, 1] at fractions (clamped, 0.25, 0.75, clamped): 512 / 2048 rounds down, 1536 / 2048 up
    assert R.resize_mask_u8(np.array([[0, 1]], np.uint8), 4, 1).tolist() == [[0, 0, 1, 1]]
