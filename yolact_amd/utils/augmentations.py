"""The image transforms of utils/augmentations.py on device.

`FastBaseTransform` — utils/augmentations.py:616-658 on device (the step right before
`Yolact.forward` in eval.py's evalimage / evalvideo, eval.py:596-597,692-695).

Same module interface: `FastBaseTransform()(img)` with img `[n, h, w, c]` float BGR on the GPU returns `[n, 3, S, S]`
normalised RGB (NCHW).  One HIP kernel (csrc/preprocess.hip) instead of permute + interpolate + normalise + index.
`to_nhwc4(img)` returns the engine's native `[n, S, S, 4]` layout directly.

`SSDAugmentation` — utils/augmentations.py:667-688, the training transform.  None of its random decisions depends on a pixel value,
so it is split in two: `draw_augmentation` makes every draw on the host, consuming the legacy numpy stream in the reference's order
(PhotometricDistort, Expand, RandomSampleCrop, RandomMirror; Resize's discard; the ground truth stays float64 numpy), and returns
an `AugmentParams` record; csrc/augment.hip then produces every output pixel with ONE gather (resize coordinate -> undo mirror ->
crop origin -> expand offset -> source pixel or fill colour -> photometric chain -> bilinear -> normalise -> RGB) and every kept
mask with a second one.  No canvas is allocated anywhere.  `SSDAugmentation.batch` does that for a list of items in two launches.

The pixel rules are OpenCV's, restated from its documentation: the 32-bit-float BGR <-> HSV formulas (cvtColor), the float
INTER_LINEAR resize for the image and the 8-bit fixed-point one (11-bit coefficients) for the masks.  cv2 is not a dependency of this
project and the rules are UNPINNED against OpenCV itself, as oracle/coco_dataset.py says of its resize.  The integer mask rule
    (ay0 * (ax0 * m00 + ax1 * m01) + ay1 * (ax0 * m10 + ax1 * m11) + 2^21) >> 22,   ax1 = round(2048 * frac), ax0 = 2048 - ax1
is this project's definition: a pixel whose exact interpolated value lies within a few 2^-11 steps of 0.5 may differ from an OpenCV
build.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from math import sqrt

import numpy as np
import torch

from .. import _lib as L
from ..config import active_cfg

MEANS = (103.94, 116.78, 123.68)     # data/config.py:28-29 (BGR order)
STD = (57.38, 57.12, 58.40)


def calc_size_preserve_ar(img_w, img_h, max_size):
    """Resize.calc_size_preserve_ar, utils/augmentations.py:132-138."""
    ratio = sqrt(img_w / img_h)
    return int(max_size * ratio), int(max_size / ratio)


def _transform_mode(cfg):
    tr = cfg.backbone.transform
    if isinstance(tr, str):          # yolact_amd.config stores the transform by name
        tr = {'resnet': dict(normalize=True, subtract_means=False, to_float=False, channel_order='RGB'),
              'vgg': dict(normalize=False, subtract_means=True, to_float=False, channel_order='RGB'),
              'darknet': dict(normalize=False, subtract_means=False, to_float=True, channel_order='RGB')}[tr]
        get = tr.get
    else:
        get = lambda k: getattr(tr, k)   # noqa: E731  (the reference's Config object)
    if get('channel_order') != 'RGB':
        raise NotImplementedError          # like augmentations.py:652-653
    if get('normalize'):
        return 0
    if get('subtract_means'):
        return 1
    if get('to_float'):
        return 2
    return 3


class FastBaseTransform(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._mean = (C.c_float * 3)(*MEANS)
        self._std = (C.c_float * 3)(*STD)

    def _run(self, img, nhwc4):
        L.require_cuda(img, 'image batch')
        cfg = active_cfg()
        if img.dim() != 4 or img.shape[3] != 3:
            raise ValueError('expected [n, h, w, 3] BGR, got %s' % (tuple(img.shape),))
        n, h, w, _ = img.shape
        if getattr(cfg, 'preserve_aspect_ratio', False):
            ow, oh = calc_size_preserve_ar(w, h, cfg.max_size)
        else:
            oh = ow = cfg.max_size
        img = img.detach().to(torch.float32).contiguous()
        out = torch.empty((n, oh, ow, 4) if nhwc4 else (n, 3, oh, ow), dtype=torch.float32, device=img.device)
        with torch.cuda.device(img.device):
            L.check(L.lib().ymi_fast_base_transform_f32(img.data_ptr(), out.data_ptr(), n, h, w, oh, ow, self._mean,
                                                        self._std, _transform_mode(cfg), 1 if nhwc4 else 0,
                                                        L.stream_ptr()), 'ymi_fast_base_transform_f32')
        return out

    def forward(self, img):
        return self._run(img, False)

    def to_nhwc4(self, img):
        return self._run(img, True)


class BaseTransform:
    """`BaseTransform` — utils/augmentations.py:601-612 (the `transform` eval.py hands COCODetection, eval.py:1097): the
    pipeline ConvertFromInts -> Resize(resize_gt=False) -> BackboneTransform(cfg.backbone.transform, mean, std, 'BGR').

    The image half is the FastBaseTransform kernel (bilinear resize with half-pixel centres, normalisation, BGR -> RGB): `img`
    is the device tensor data.jpeg.imread returned (uint8 / float BGR [h,w,3]; a numpy array is uploaded) and comes back as a
    float32 [S,S,3] device view (HWC like the reference's array, so `.permute(2, 0, 1)` gives the network input).
    cv2.resize and this kernel evaluate the same bilinear formula in fp32 but round the sample coordinate differently
    (cv2: double -> float; here: fp32 throughout, as F.interpolate), so values agree to ~1e-5 of the normalised range, not
    bit for bit.  The ground-truth half is the reference's host code: `Resize(resize_gt=False)` leaves masks / boxes at
    their size and drops boxes narrower than cfg.discard_box_width / height (utils/augmentations.py:170-178)."""

    def __init__(self, mean=MEANS, std=STD):
        self._fbt = FastBaseTransform()
        self._fbt._mean = (C.c_float * 3)(*mean)
        self._fbt._std = (C.c_float * 3)(*std)

    def __call__(self, img, masks=None, boxes=None, labels=None):
        import numpy as np
        cfg = active_cfg()
        if not torch.is_tensor(img):
            img = torch.from_numpy(np.ascontiguousarray(img))
        if not img.is_cuda:
            if not torch.cuda.is_available():
                L.require_cuda(img, 'image')
            img = img.cuda()
        out = self._fbt(img.unsqueeze(0))[0].permute(1, 2, 0)      # [S,S,3] view of the NCHW result
        if boxes is not None and labels is not None:
            w = boxes[:, 2] - boxes[:, 0]
            h = boxes[:, 3] - boxes[:, 1]
            keep = (w > getattr(cfg, 'discard_box_width', 4 / 550)) * (h > getattr(cfg, 'discard_box_height', 4 / 550))
            # (device masks, COCODetection(device_masks=True): the index goes where the masks are)
            masks = masks[torch.from_numpy(np.asarray(keep, dtype=bool)).to(masks.device)] if torch.is_tensor(masks) else masks[keep]
            boxes = boxes[keep]
            labels['labels'] = labels['labels'][keep]
            labels['num_crowds'] = (labels['labels'] < 0).sum()
        return out, masks, boxes, labels


# ---- SSDAugmentation: the draws (host) ---------------------------------------------------------------------------------------

# RandomSampleCrop's options (utils/augmentations.py:293-303): None = keep the whole image, else (min IoU, max IoU)
_CROP_OPTIONS = (None, (0.1, None), (0.3, None), (0.7, None), (0.9, None), (None, None))
_CROP_TRIALS = 50


@dataclass
class AugmentParams:
    """Everything `draw_augmentation` decided for one image; what csrc/augment.hip needs besides the pixels.  A stage that was not
    drawn is None / False (the kernel SKIPS it, it does not apply a neutral value)."""
    height: int                        # the source image
    width: int
    photometric: bool = False          # PhotometricDistort ran: the BGR -> HSV -> BGR round trip happens even if nothing was drawn
    brightness: float = None           # + delta
    contrast: float = None             # * alpha ...
    contrast_last: bool = False        # ... after the HSV stages (the reference's pd[1:]) instead of before them (pd[:-1])
    saturation: float = None           # S *= sat
    hue: float = None                  # H += hue, wrapped once
    canvas_h: int = 0                  # Expand's canvas (= the source size without an expansion) ...
    canvas_w: int = 0
    off_x: int = 0                     # ... and where the source's corner lies in it
    off_y: int = 0
    crop: tuple = (0, 0, 0, 0)         # x0, y0, x1, y1 in the canvas (the whole canvas without a crop)
    mirror: bool = False
    keep: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))   # surviving ground-truth rows, in order

    @property
    def crop_h(self):
        return self.crop[3] - self.crop[1]

    @property
    def crop_w(self):
        return self.crop[2] - self.crop[0]


def _refuse_unsupported(cfg):
    for name in ('augment_random_flip', 'use_gt_bboxes', 'preserve_aspect_ratio'):
        if getattr(cfg, name, False):
            raise NotImplementedError('SSDAugmentation: cfg.%s is not supported (no shipped config sets it)' % name)


def _rect_iou(boxes, rect):
    """IoU of every row of `boxes` with the integer rect, in jaccard_numpy's op order (utils/augmentations.py:12-36)."""
    hi = np.minimum(boxes[:, 2:], rect[2:])
    lo = np.maximum(boxes[:, :2], rect[:2])
    ext = np.clip(hi - lo, a_min=0, a_max=np.inf)
    inter = ext[:, 0] * ext[:, 1]
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    area_rect = (rect[2] - rect[0]) * (rect[3] - rect[1])
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / (area + area_rect - inter)


def _draw_crop(height, width, boxes, num_crowds, rng):
    """RandomSampleCrop.__call__ (utils/augmentations.py:305-405) without the pixels -> (rect | None, kept mask | None)."""
    while True:
        mode = _CROP_OPTIONS[rng.choice(len(_CROP_OPTIONS))]
        if mode is None:
            return None, None
        min_iou = float('-inf') if mode[0] is None else mode[0]
        max_iou = float('inf') if mode[1] is None else mode[1]
        for _ in range(_CROP_TRIALS):
            w = rng.uniform(0.3 * width, width)
            h = rng.uniform(0.3 * height, height)
            if h / w < 0.5 or h / w > 2:
                continue
            left = rng.uniform(width - w)          # the reference's call: low = width - w, high = 1.0
            top = rng.uniform(height - h)
            rect = np.array([int(left), int(top), int(left + w), int(top + h)])
            overlap = _rect_iou(boxes, rect)
            # the reference's own comment calls this test bugged and keeps it (it halves mAP when "fixed")
            if overlap.min() < min_iou and max_iou < overlap.max():
                continue
            centers = (boxes[:, :2] + boxes[:, 2:]) / 2.0
            inside = (rect[0] < centers[:, 0]) * (rect[1] < centers[:, 1]) * ((rect[2] > centers[:, 0]) * (rect[3] > centers[:, 1]))
            crowd = np.zeros(inside.shape, dtype=np.int32)
            if num_crowds > 0:
                crowd[-num_crowds:] = 1
            if not inside.any() or np.sum(1 - crowd[inside]) == 0:      # nothing left, or only crowds
                continue
            return rect, inside


def draw_augmentation(height, width, boxes, labels, cfg=None, rng=np.random):
    """Every random decision of the reference's SSDAugmentation for an image of (height, width) with relative `boxes` [n,4] and
    `labels` = {'labels': [n], 'num_crowds': k}, drawn from `rng` (the legacy numpy stream) in the reference's order
    -> (AugmentParams, boxes [m,4] float64 relative to the S x S output, {'labels': [m], 'num_crowds': k'}).
    The inputs are not modified (the reference transforms them in place)."""
    cfg = active_cfg() if cfg is None else cfg
    _refuse_unsupported(cfg)
    height, width = int(height), int(width)
    S = int(cfg.max_size)
    boxes = np.array(boxes, dtype=np.float64)
    lab = np.array(labels['labels'])
    num_crowds = labels['num_crowds']
    keep = np.arange(boxes.shape[0])
    p = AugmentParams(height=height, width=width)

    # ToAbsoluteCoords
    boxes[:, 0] *= width
    boxes[:, 2] *= width
    boxes[:, 1] *= height
    boxes[:, 3] *= height

    if getattr(cfg, 'augment_photometric_distort', True):       # PhotometricDistort, utils/augmentations.py:504-525
        p.photometric = True
        if rng.randint(2):
            p.brightness = rng.uniform(-32, 32)
        p.contrast_last = not rng.randint(2)
        if not p.contrast_last and rng.randint(2):
            p.contrast = rng.uniform(0.5, 1.5)
        if rng.randint(2):
            p.saturation = rng.uniform(0.5, 1.5)
        if rng.randint(2):
            p.hue = rng.uniform(-18.0, 18.0)
        if p.contrast_last and rng.randint(2):
            p.contrast = rng.uniform(0.5, 1.5)

    h, w = height, width
    if getattr(cfg, 'augment_expand', True) and not rng.randint(2):       # Expand, utils/augmentations.py:408-440
        ratio = rng.uniform(1, 4)
        left = rng.uniform(0, w * ratio - w)
        top = rng.uniform(0, h * ratio - h)
        p.off_x, p.off_y = int(left), int(top)
        boxes[:, :2] += (p.off_x, p.off_y)
        boxes[:, 2:] += (p.off_x, p.off_y)
        h, w = int(h * ratio), int(w * ratio)
    p.canvas_h, p.canvas_w = h, w

    rect = None
    if getattr(cfg, 'augment_random_sample_crop', True):
        rect, inside = _draw_crop(h, w, boxes, num_crowds, rng)
    if rect is not None:
        if num_crowds > 0:
            crowd = np.zeros(inside.shape, dtype=np.int32)
            crowd[-num_crowds:] = 1
            num_crowds = np.sum(crowd[inside])
        boxes, lab, keep = boxes[inside, :].copy(), lab[inside], keep[inside]
        boxes[:, :2] = np.maximum(boxes[:, :2], rect[:2])
        boxes[:, :2] -= rect[:2]
        boxes[:, 2:] = np.minimum(boxes[:, 2:], rect[2:])
        boxes[:, 2:] -= rect[:2]
        # the rect lies inside the canvas: left <= max(width - w, 1) and w <= width, so int(left + w) <= width; rows likewise
        p.crop = tuple(int(v) for v in rect)
        h, w = p.crop_h, p.crop_w
    else:
        p.crop = (0, 0, w, h)

    if getattr(cfg, 'augment_random_mirror', True) and rng.randint(2):    # RandomMirror
        p.mirror = True
        boxes = boxes.copy()
        boxes[:, 0::2] = w - boxes[:, 2::-2]

    # Resize (resize_gt=True): the discard test sees ABSOLUTE coordinates, as in the reference
    boxes[:, [0, 2]] *= (S / w)
    boxes[:, [1, 3]] *= (S / h)
    bw = boxes[:, 2] - boxes[:, 0]
    bh = boxes[:, 3] - boxes[:, 1]
    ok = (bw > getattr(cfg, 'discard_box_width', 4 / 550)) * (bh > getattr(cfg, 'discard_box_height', 4 / 550))
    boxes, lab, keep = boxes[ok], lab[ok], keep[ok]
    num_crowds = (lab < 0).sum()

    # ToPercentCoords on the S x S image
    boxes[:, 0] /= S
    boxes[:, 2] /= S
    boxes[:, 1] /= S
    boxes[:, 3] /= S
    p.keep = keep.astype(np.int64)
    return p, boxes, {'num_crowds': num_crowds, 'labels': lab}


# ---- SSDAugmentation: the pixels (device) ------------------------------------------------------------------------------------

def _params_flags(p):
    f = L.AUG_PHOTOMETRIC if p.photometric else 0
    f |= L.AUG_BRIGHTNESS if p.brightness is not None else 0
    f |= L.AUG_CONTRAST if p.contrast is not None else 0
    f |= L.AUG_CONTRAST_LAST if p.contrast_last else 0
    f |= L.AUG_SATURATION if p.saturation is not None else 0
    f |= L.AUG_HUE if p.hue is not None else 0
    f |= L.AUG_MIRROR if p.mirror else 0
    return f


def _device_image(img, device=None):
    """[h,w,3] BGR, uint8 or float, numpy or tensor -> contiguous device tensor (uint8 stays uint8, anything else -> float32)."""
    if not torch.is_tensor(img):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError('expected an [h, w, 3] BGR image, got %s' % (tuple(img.shape),))
    if not img.is_cuda:
        if not torch.cuda.is_available():
            L.require_cuda(img, 'image')
        img = img.cuda() if device is None else img.to(device)
    if img.dtype != torch.uint8:
        img = img.to(torch.float32)
    return img.detach().contiguous()


def _device_masks(masks, h, w, device):
    """[n,h,w] instance masks (annToMask's uint8 0 / 1), numpy or tensor -> contiguous uint8 device tensor, or None."""
    if masks is None:
        return None
    if not torch.is_tensor(masks):
        masks = torch.from_numpy(np.ascontiguousarray(masks, dtype=np.uint8))
    if masks.dim() != 3 or tuple(masks.shape[1:]) != (h, w):
        raise ValueError('expected [n, %d, %d] masks, got %s' % (h, w, tuple(masks.shape)))
    return masks.to(device=device, dtype=torch.uint8).contiguous()


class SSDAugmentation:
    """`SSDAugmentation` — utils/augmentations.py:667-688, the transform the reference trains with
    (`COCODetection(transform=SSDAugmentation(MEANS))`, train.py).  Same constructor and call signature; the draws come from
    `numpy.random` in the reference's order (`draw_augmentation`), the pixels from csrc/augment.hip.

    `__call__(img, masks, boxes, labels)` -> (img float32 [S,S,3] device view of the CHW result, masks float32 [n,S,S] on the
    device, boxes float64 [n,4] ndarray, {'labels', 'num_crowds'}).  `img` is the device tensor data.jpeg.imread returns (uint8 or
    float BGR [h,w,3]; a numpy array is uploaded), `masks` a uint8 [n,h,w] ndarray or device tensor.
    `batch(items)` augments a list of such tuples in two launches."""

    def __init__(self, mean=MEANS, std=STD):
        self.mean = tuple(float(v) for v in mean)
        self.std = tuple(float(v) for v in std)

    def __call__(self, img, masks, boxes, labels):
        cfg = active_cfg()
        _refuse_unsupported(cfg)
        img = _device_image(img)
        p, boxes, labels = draw_augmentation(img.shape[0], img.shape[1], boxes, labels, cfg)
        out, mk = self.apply([(img, masks, p)], cfg=cfg)
        return out[0].permute(1, 2, 0), mk[0], boxes, labels

    def batch(self, items, nhwc4=False, masks_u8=False):
        """items: [(img, masks, boxes, labels), ...] as `__call__` takes them -> (images [B,3,S,S] float32, or [B,S,S,4] with nhwc4;
        targets: per image a float32 [n_i,5] device tensor (boxes, label); masks: per image [n_i,S,S] float32 (uint8 with masks_u8);
        num_crowds: per image an int) — what Yolact.forward_train and MultiBoxLoss take.  All draws happen first, on the host, image
        by image in list order; then one launch for all images and one for all masks.
        An item whose boxes Resize's discard all drops comes back with targets [0,5] and masks [0,S,S]: COCODetection.pull_item
        resamples another item in that case (as the reference does) and MultiBoxLoss does not take an empty target, so a caller that
        can meet such items filters them out (`t.shape[0] == 0`) before the loss."""
        cfg = active_cfg()
        _refuse_unsupported(cfg)
        work, targets, num_crowds = [], [], []
        for img, masks, boxes, labels in items:
            img = _device_image(img)
            p, boxes, labels = draw_augmentation(img.shape[0], img.shape[1], boxes, labels, cfg)
            work.append((img, masks, p))
            targets.append(np.hstack((boxes, np.asarray(labels['labels'], dtype=np.float64)[:, None])))
            num_crowds.append(int(labels['num_crowds']))
        images, masks = self.apply(work, nhwc4=nhwc4, masks_u8=masks_u8, cfg=cfg)
        targets = [torch.as_tensor(t, dtype=torch.float32).to(images.device) for t in targets]
        return images, targets, masks, num_crowds

    def apply(self, work, nhwc4=False, masks_u8=False, cfg=None):
        """The device half alone: work = [(img, masks, AugmentParams), ...] -> (images, [masks of image i: [len(keep_i),S,S]]).
        `params.keep` lists the instances to transform, in output order; the others are never read."""
        cfg = active_cfg() if cfg is None else cfg
        S, B = int(cfg.max_size), len(work)
        if B == 0:
            raise ValueError('SSDAugmentation: an empty batch')
        recs = (L.AugmentRec * B)()
        hold, kept, counts = [], [], []
        device = None
        for b, (img, masks, p) in enumerate(work):
            img = _device_image(img, device)
            device = img.device
            h, w = int(img.shape[0]), int(img.shape[1])
            if (h, w) != (p.height, p.width):
                raise ValueError('the parameters were drawn for a %d x %d image, this one is %d x %d' % (p.height, p.width, h, w))
            keep = [int(k) for k in p.keep]
            mk = _device_masks(masks, h, w, device) if keep else None
            if keep and mk is None:
                raise ValueError('image %d keeps %d instances but has no masks' % (b, len(keep)))
            hold += [img, mk]
            r = recs[b]
            r.src, r.masks = img.data_ptr(), (mk.data_ptr() if mk is not None else None)
            r.h, r.w, r.n_inst = h, w, (int(mk.shape[0]) if mk is not None else 0)
            r.flags = _params_flags(p) | (0 if img.dtype == torch.uint8 else L.AUG_SRC_F32)
            r.canvas_h, r.canvas_w, r.off_x, r.off_y = p.canvas_h, p.canvas_w, p.off_x, p.off_y
            r.crop_x0, r.crop_y0, r.crop_x1, r.crop_y1 = p.crop
            r.delta = p.brightness if p.brightness is not None else 0.0
            r.alpha = p.contrast if p.contrast is not None else 1.0
            r.sat = p.saturation if p.saturation is not None else 1.0
            r.hue = p.hue if p.hue is not None else 0.0
            r.out_slot, r.mask_first, r.n_kept, r.kept_first = b, len(kept), len(keep), len(kept)
            kept += keep
            counts.append(len(keep))
        n_masks = len(kept)
        kept_arr = (C.c_int32 * max(n_masks, 1))(*kept)
        d = L.AugmentDesc()
        d.recs, d.kept = recs, C.cast(kept_arr, C.c_void_p)
        d.B, d.S, d.n_masks, d.mode, d.out_nhwc4, d.masks_u8 = B, S, n_masks, _transform_mode(cfg), int(bool(nhwc4)), int(bool(masks_u8))
        d.mean_bgr, d.std_bgr = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std)
        lib = L.lib()
        with torch.cuda.device(device):
            out = torch.empty((B, S, S, 4) if nhwc4 else (B, 3, S, S), dtype=torch.float32, device=device)
            mout = torch.empty((n_masks, S, S), dtype=torch.uint8 if masks_u8 else torch.float32, device=device)
            d.ws_bytes = lib.ymi_workspace_bytes(L.WS_AUGMENT, C.byref(d))
            ws = torch.empty(max(int(d.ws_bytes), 16), dtype=torch.uint8, device=device)
            d.out, d.masks_out, d.ws = out.data_ptr(), (mout.data_ptr() if n_masks else None), ws.data_ptr()
            L.check(lib.ymi_ssd_augment_f32(C.byref(d), L.stream_ptr()), 'ymi_ssd_augment_f32')
        del hold
        return out, list(torch.split(mout, counts))
