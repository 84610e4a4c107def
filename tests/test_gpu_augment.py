"""SSDAugmentation on the GPU (csrc/augment.hip: ymi_ssd_augment_f32; yolact_amd/utils/augmentations.py) against the numpy
restatement of the reference's step-by-step pipeline (tests/augment_ref.py).

Sources of 37 x 53 and 64 x 48 to S = 24 and 40: odd sizes, a downscale and an upscale, both borders clamped, more than one block.
IMAGE BOUND: the kernel is compared with the float64 restatement; the bound is 4 x the largest deviation of the float32 restatement
from the float64 one over the same cases (the factor covers fused multiply-adds and the device's division), computed here on the
CPU, and never more than the 2e-3 of the normalised range tests/test_gpu_jpeg.py allows BaseTransform.
Measured on an MI355X: see the comment at IMAGE_BOUND below.  MASKS are exact: the integer rule has no rounding to bound.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import augment_ref as R
import coco_synth
import yolact_amd
from yolact_amd import _lib as L
from yolact_amd.config import CONFIGS, active_cfg
from yolact_amd.utils.augmentations import MEANS, STD, AugmentParams, SSDAugmentation, draw_augmentation

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SOURCES = ((37, 53), (64, 48))
SIZES = (24, 40)


def cfg_for(S, config='yolact_base_config'):
    return CONFIGS[config].copy({'max_size': S})


@functools.lru_cache(maxsize=None)
def source(h, w, as_float=False):
    """A random BGR image with the pixels the photometric edge cases need in its first row: black (brightness -32 -> negative V),
    saturated primaries (saturation 1.5 -> negative channels), reds a few degrees either side of H = 0 / 360 (the hue wrap), grey."""
    rng = np.random.RandomState(h * 100 + w)
    img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    img[0, :9] = [[0, 0, 0], [0, 0, 255], [0, 255, 0], [255, 0, 0], [10, 0, 255], [0, 10, 255], [128, 128, 128], [255, 255, 255],
                  [0, 0, 1]]
    img[-1, -3:] = [[0, 0, 0], [20, 0, 250], [0, 20, 250]]
    if as_float:
        return (img.astype(np.float32) + rng.rand(h, w, 3).astype(np.float32) * 0.75).astype(np.float32)
    return img


def stage_cases(h, w):
    """name -> AugmentParams, one stage at a time, then all together."""
    P = functools.partial(AugmentParams, height=h, width=w, canvas_h=h, canvas_w=w, crop=(0, 0, w, h))
    ch, cw = h + 9, w + 11
    geo = dict(canvas_h=ch, canvas_w=cw, off_x=11, off_y=9, crop=(5, 3, cw - 2, ch - 4), mirror=True)
    return {
        'identity': P(),
        'mirror': P(mirror=True),
        'crop_two_edges': P(crop=(w // 3, 0, w, (2 * h) // 3)),                         # touches the top and the right edge
        'expand_corner': P(canvas_h=ch, canvas_w=cw, off_x=11, off_y=9, crop=(0, 0, cw, ch)),   # source in the bottom-right corner
        'expand_crop_in_fill': P(canvas_h=ch, canvas_w=cw, off_x=0, off_y=0, crop=(w - 4, h - 5, cw, ch)),   # mostly fill
        'round_trip_only': P(photometric=True),
        'brightness': P(photometric=True, brightness=20.5),
        'brightness_dark': P(photometric=True, brightness=-32.0),                        # black pixels: V = -32
        'contrast_first': P(photometric=True, contrast=1.3),
        'contrast_last': P(photometric=True, contrast=0.7, contrast_last=True),
        'saturation_high': P(photometric=True, saturation=1.5),                          # saturated pixels: negative channels
        'saturation_low': P(photometric=True, saturation=0.5, contrast_last=True),
        'hue_up': P(photometric=True, hue=17.0),                                         # wraps past 360
        'hue_down': P(photometric=True, hue=-17.5, contrast_last=True),                  # wraps below 0
        'all_contrast_first': P(photometric=True, brightness=-11.25, contrast=1.45, saturation=1.4, hue=-18.0, **geo),
        'all_contrast_last': P(photometric=True, brightness=31.0, contrast=0.55, contrast_last=True, saturation=0.6, hue=18.0,
                               **geo),
    }


def all_cases():
    """(name, image, params, S, config) of every image comparison."""
    for h, w in SOURCES:
        for S in SIZES:
            for name, p in stage_cases(h, w).items():
                yield '%dx%d->%d %s' % (h, w, S, name), source(h, w), p, S, 'yolact_base_config'
            both = stage_cases(h, w)['all_contrast_first']
            yield '%dx%d->%d float source' % (h, w, S), source(h, w, True), both, S, 'yolact_base_config'
            yield '%dx%d->%d to_float' % (h, w, S), source(h, w), both, S, 'yolact_darknet53_config'


MODES = {'yolact_base_config': 0, 'yolact_darknet53_config': 2}


@functools.lru_cache(maxsize=None)
def references():
    """name -> (float64 restatement, its deviation from the float32 one), computed once and shared."""
    out = {}
    for name, img, p, S, config in all_cases():
        r64 = R.augment_image(img, p, S, MEANS, STD, MODES[config], np.float64)
        r32 = R.augment_image(img, p, S, MEANS, STD, MODES[config], np.float32)
        assert r32.dtype == np.float32 and r64.dtype == np.float64
        out[name] = (r64, float(np.abs(r32.astype(np.float64) - r64).max()))
    return out


def image_bound():
    return 4 * max(dev for _, dev in references().values())


def run_image(img, p, S, config='yolact_base_config', nhwc4=False):
    out, _ = SSDAugmentation().apply([(img, None, p)], nhwc4=nhwc4, cfg=cfg_for(S, config))
    return out


# IMAGE_BOUND, measured (normalised units): the float32 restatement is 4.053e-06 from the float64 one over the cases above (worst:
# 37x53->40 all_contrast_first), so the bound is 1.621e-05; the kernel's largest distance from the float64 restatement on an MI355X is
# 4.053e-06, the float32 restatement's own (the kernel rounds where it does).  profiles/augment_probe_b8.txt holds the same figures.
def test_image_parity_one_stage_at_a_time_then_all_together():
    refs = references()
    bound = image_bound()
    assert 0 < bound <= 2e-3, bound
    worst = {}
    for name, img, p, S, config in all_cases():
        got = run_image(img, p, S, config)
        assert tuple(got.shape) == (1, 3, S, S) and got.dtype == torch.float32
        got = got[0].permute(1, 2, 0).cpu().numpy().astype(np.float64)
        worst[name] = float(np.abs(got - refs[name][0]).max())
    dev = max(d for _, d in refs.values())
    print('float32 restatement vs float64: %.3e; bound %.3e; kernel vs float64: %.3e (worst case %s)'
          % (dev, bound, max(worst.values()), max(worst, key=worst.get)))
    bad = {k: v for k, v in worst.items() if not v <= bound}
    assert not bad, (bound, bad)


def test_identity_agrees_with_the_fast_base_transform_oracle():
    """No stage drawn = Resize + BackboneTransform: the FastBaseTransform oracle (F.interpolate, which rounds the sample coordinate in
    fp32 where cv2 rounds a double), to the bound tests/test_fast_base_transform.py gives that kernel."""
    from oracle import yolact_oracle
    for h, w in SOURCES:
        for S in SIZES:
            img = source(h, w)
            ref = yolact_oracle.fast_base_transform(torch.from_numpy(img.astype(np.float32))[None], cfg_for(S))
            got = run_image(img, stage_cases(h, w)['identity'], S).cpu()
            assert got.shape == ref.shape
            assert (got - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item()), (h, w, S)


def masks_for(h, w):
    """4 instances: two blobs, one that lies entirely in the area the crop below removes, one that covers everything."""
    m = np.zeros((4, h, w), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    m[0] = ((yy - h * 0.45) ** 2 / (h * 0.30) ** 2 + (xx - w * 0.5) ** 2 / (w * 0.35) ** 2) < 1
    m[1, :4, :5] = 1                                             # top-left corner: cropped away
    m[2] = ((yy + xx) % 7 < 3) & (yy > h // 3)
    m[3] = 1
    return m


def mask_params(h, w, keep):
    ch, cw = h + 7, w + 12
    return AugmentParams(height=h, width=w, canvas_h=ch, canvas_w=cw, off_x=6, off_y=2, crop=(6 + 5, 2 + 4, cw - 3, ch - 1), mirror=True,
                         keep=np.array(keep, dtype=np.int64))


@pytest.mark.parametrize('masks_u8', [False, True])
def test_masks_are_exact(masks_u8):
    for h, w in SOURCES:
        for S in SIZES:
            m = masks_for(h, w)
            for p in (mask_params(h, w, [2, 0, 3, 1]),                                   # reordered; 1 is kept but cropped away
                      AugmentParams(height=h, width=w, canvas_h=h, canvas_w=w, crop=(0, 0, w, h), keep=np.array([3, 0]))):
                ref = R.augment_masks(m, p, S)
                for src in (m, torch.from_numpy(m).to(DEV)):
                    _, got = SSDAugmentation().apply([(source(h, w), src, p)], masks_u8=masks_u8, cfg=cfg_for(S))
                    assert got[0].dtype == (torch.uint8 if masks_u8 else torch.float32) and tuple(got[0].shape) == ref.shape
                    assert np.array_equal(got[0].cpu().numpy(), ref.astype(got[0].cpu().numpy().dtype)), (h, w, S)
            ref = R.augment_masks(m, mask_params(h, w, [2, 0, 3, 1]), S)
            assert ref[3].max() == 0 and ref[2].min() == 0 and ref[2].max() == 1 and ref[0].any()     # the cases are what they claim


def test_batch_of_three_equals_the_single_calls_bit_for_bit():
    S = 40
    cfg = cfg_for(S)
    (h0, w0), (h1, w1) = SOURCES
    work = [(source(h0, w0), masks_for(h0, w0), mask_params(h0, w0, [3, 0])),
            (source(h1, w1), masks_for(h1, w1), AugmentParams(height=h1, width=w1, photometric=True, hue=9.0, canvas_h=h1, canvas_w=w1,
                                                               crop=(3, 2, w1 - 1, h1), keep=np.array([1, 2, 0]))),       # no expand
            (source(h0, w0, True), None, stage_cases(h0, w0)['all_contrast_last'])]                                      # no masks kept
    aug = SSDAugmentation()
    for nhwc4 in (False, True):
        imgs, masks = aug.apply(work, nhwc4=nhwc4, cfg=cfg)
        again, masks_again = aug.apply(work, nhwc4=nhwc4, cfg=cfg)
        assert tuple(imgs.shape) == ((3, S, S, 4) if nhwc4 else (3, 3, S, S))
        assert torch.equal(imgs, again) and all(torch.equal(a, b) for a, b in zip(masks, masks_again))
        assert [tuple(m.shape) for m in masks] == [(2, S, S), (3, S, S), (0, S, S)]
        for i, item in enumerate(work):
            one, one_masks = aug.apply([item], nhwc4=nhwc4, cfg=cfg)
            assert torch.equal(one[0], imgs[i]), i
            assert torch.equal(one_masks[0], masks[i]), i
        if nhwc4:
            assert imgs[..., 3].abs().max().item() == 0
            assert torch.equal(imgs[..., :3].permute(0, 3, 1, 2), nchw)
        else:
            nchw = imgs


def test_bad_records_return_the_error_and_launch_nothing():
    lib = L.lib()
    S, h, w = 24, 37, 53
    img = torch.from_numpy(source(h, w)).to(DEV)
    m = torch.from_numpy(masks_for(h, w)).to(DEV)
    out = torch.full((1, 3, S, S), 7.0, device=DEV)
    mout = torch.full((2, S, S), 7.0, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)

    def call(kept=(0, 1), **kw):
        rec = L.AugmentRec(src=img.data_ptr(), masks=m.data_ptr(), h=h, w=w, n_inst=4, flags=0, canvas_h=h, canvas_w=w, off_x=0, off_y=0,
                           crop_x0=0, crop_y0=0, crop_x1=w, crop_y1=h, delta=0, alpha=1, sat=1, hue=0, out_slot=0, mask_first=0,
                           n_kept=2, kept_first=0)
        top = {}
        for k, v in kw.items():
            if k in dict(L.AugmentRec._fields_):
                setattr(rec, k, v)
            else:
                top[k] = v
        recs = (L.AugmentRec * 1)(rec)
        kept_arr = (C.c_int32 * 2)(*kept)
        d = L.AugmentDesc(recs=recs, kept=C.cast(kept_arr, C.c_void_p), out=out.data_ptr(), masks_out=mout.data_ptr(), ws=ws.data_ptr(),
                          ws_bytes=ws.numel(), B=1, S=S, n_masks=2, mode=0, out_nhwc4=0, masks_u8=0)
        d.mean_bgr, d.std_bgr = (C.c_float * 3)(*MEANS), (C.c_float * 3)(*STD)
        for k, v in top.items():
            setattr(d, k, v)
        rc = lib.ymi_ssd_augment_f32(C.byref(d), L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    EARG, ESHAPE, ENULL = -1, -2, -3
    assert call(crop_x1=w + 1) == ESHAPE                          # the crop leaves the canvas
    assert call(crop_y0=-1) == ESHAPE
    assert call(kept=(0, 4)) == ESHAPE                            # an index beyond n
    assert call(kept=(-1, 0)) == ESHAPE
    assert call(canvas_w=w + 4, crop_x1=w + 4, off_x=5) == ESHAPE   # the source leaves the canvas
    assert call(crop_x1=0) == EARG and call(h=0) == EARG and call(S=0) == EARG and call(mode=4) == EARG
    assert call(src=None) == ENULL and call(masks=None) == ENULL and call(ws=None) == ENULL
    assert call(out=out.data_ptr() + 4, out_nhwc4=1) == ESHAPE          # the NHWC-4 store is 16 bytes wide
    assert call(ws_bytes=64) == ESHAPE and call(out_slot=1) == ESHAPE and call(mask_first=1) == ESHAPE and call(n_kept=1) == ESHAPE
    assert bool((out == 7).all()) and bool((mout == 7).all()) and not bool(ws.any())      # nothing was launched or copied
    assert call() == 0
    assert not bool((out == 7).any()) and not bool((mout == 7).any())


def _with_max_size(S):
    """The config object the transform reads at call time, with max_size = S; returns (cfg, restore)."""
    yolact_amd.set_cfg('yolact_resnet50_config')
    cfg = active_cfg()
    was = cfg.max_size
    cfg.max_size = S

    def restore():
        cfg.max_size = was
    return cfg, restore


def test_coco_detection_with_the_training_transform(tmp_path):
    from yolact_amd.data import COCODetection, detection_collate
    S = 40
    cfg, restore = _with_max_size(S)
    try:
        info_file = coco_synth.write_dataset(str(tmp_path))
        ds = COCODetection(str(tmp_path), info_file, transform=SSDAugmentation())
        plain = COCODetection(str(tmp_path), info_file, transform=None)
        items = []
        for idx in range(len(ds)):
            raw_img, raw_target, raw_masks, h, w, raw_crowds = plain.pull_item(idx)
            np.random.seed(100 + idx)
            img, target, masks, h2, w2, num_crowds = ds.pull_item(idx)
            np.random.seed(100 + idx)                               # the host replay of the same draws
            p, boxes, labels = draw_augmentation(h, w, raw_target[:, :4], {'num_crowds': raw_crowds, 'labels': raw_target[:, 4]}, cfg)
            assert len(boxes) > 0, 'the fixed seed was chosen so that no item is resampled'
            assert (h2, w2) == (h, w) and img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (3, S, S)
            assert masks.is_cuda and masks.dtype == torch.float32 and tuple(masks.shape) == (len(boxes), S, S)
            assert target.dtype == np.float64 and np.array_equal(target, np.hstack((boxes, labels['labels'][:, None])))
            assert int(num_crowds) == int(labels['num_crowds'])
            assert np.array_equal(masks.cpu().numpy(), R.augment_masks(raw_masks, p, S).astype(np.float32))
            ref = R.augment_image(raw_img.permute(1, 2, 0).cpu().numpy(), p, S, MEANS, STD, 0, np.float64)
            assert np.abs(img.permute(1, 2, 0).cpu().numpy() - ref).max() <= 2e-3
            items.append((img, (target, masks, num_crowds)))
        imgs, (targets, gt_masks, crowds) = detection_collate(items)
        assert len(imgs) == len(ds) and all(t.dtype == torch.float32 and t.shape[1] == 5 for t in targets)
        assert all(m.is_cuda and m.dtype == torch.float32 for m in gt_masks) and len(crowds) == len(ds)
    finally:
        restore()


def test_batch_feeds_forward_train_and_the_loss(tmp_path):
    """SSDAugmentation.batch -> Yolact.forward_train -> MultiBoxLoss at max_size = 64, the training step's data flow."""
    from yolact_amd.data import COCODetection
    from yolact_amd.layers.modules import MultiBoxLoss
    from yolact_amd.yolact import Yolact
    S = 64
    before = yolact_amd.config.cfg.copy()
    cfg, restore = _with_max_size(S)
    try:
        info_file = coco_synth.write_dataset(str(tmp_path))
        plain = COCODetection(str(tmp_path), info_file, transform=None)
        items = []
        for idx in (0, 1):
            raw_img, raw_target, raw_masks, h, w, raw_crowds = plain.pull_item(idx)
            items.append((raw_img.permute(1, 2, 0).contiguous(), raw_masks, raw_target[:, :4], {'num_crowds': raw_crowds, 'labels': raw_target[:, 4]}))
        np.random.seed(11)
        images, targets, masks, num_crowds = SSDAugmentation().batch(items)
        np.random.seed(11)
        nhwc, targets2, _, _ = SSDAugmentation().batch(items, nhwc4=True, masks_u8=True)
        assert tuple(images.shape) == (2, 3, S, S) and images.dtype == torch.float32 and tuple(nhwc.shape) == (2, S, S, 4)
        assert torch.equal(nhwc[..., :3].permute(0, 3, 1, 2), images) and all(torch.equal(a, b) for a, b in zip(targets, targets2))
        for t, m, c in zip(targets, masks, num_crowds):
            assert t.is_cuda and t.dtype == torch.float32 and t.shape[1] == 5 and tuple(m.shape) == (t.shape[0], S, S)
            assert m.dtype == torch.float32 and isinstance(c, int) and int((t[:, 4] < 0).sum()) == c
        torch.manual_seed(0)
        net = Yolact()
        for mod in (net.backbone, net.fpn, net.proto_net, net.prediction_layers, net.semantic_seg_conv):
            mod.to(DEV)
        pred = net.forward_train(images)
        assert pred['loc'].shape[0] == 2 and bool(torch.isfinite(pred['loc']).all())
        losses = MultiBoxLoss(cfg.num_classes, 0.5, 0.4, 3)(None, pred, targets, masks, num_crowds)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    finally:
        restore()
        yolact_amd.config.cfg.replace(before)
