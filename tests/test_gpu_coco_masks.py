"""COCO ground-truth masks rasterised on the GPU (csrc/coco_mask.hip, yolact_amd.data.ann_to_masks_device) against BOTH
restatements of pycocotools' maskApi.c: the host codec (`ann_to_mask`, csrc/coco_host.cpp) and the Python one
(oracle/coco_mask.py).  Equality is exact everywhere; every call writes into a buffer pre-filled with 0xAB with guard bytes
around every mask (and masks at every alignment), and runs twice.  Cases are batched into few calls: one call takes annotations
of any mix of kinds and image sizes."""
import ctypes as C

import numpy as np
import pytest
import torch

import ap_eval_ref as APR
import coco_synth
import yolact_amd
from oracle import coco_mask, coco_rle
from yolact_amd import _lib as L
from yolact_amd.config import active_cfg
from yolact_amd.data import COCODetection, COCOIndex, ann_to_mask, ann_to_masks_device
from yolact_amd.data import coco as DC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 13            # odd: the masks of one call start at every alignment mod 4


def raster(anns, sizes):
    """One ymi_coco_masks_u8 call -> the masks as numpy arrays; the guards and the 'every byte is written' property are
    checked here, for every case of this file."""
    pk = DC.pack_annotations(anns, sizes)
    n = len(anns)
    offs, total = [], GUARD
    for h, w in sizes:
        offs.append(total)
        total += h * w + GUARD
    buf = torch.full((total,), 0xAB, dtype=torch.uint8, device=DEV)
    recs = (L.CocoMaskRec * n)()
    for i in range(n):
        r = recs[i]
        r.out = buf.data_ptr() + offs[i]
        r.kind, r.h, r.w, r.n, r.first, r.xy_first = (int(v[i]) for v in (pk.kind, pk.h, pk.w, pk.n, pk.first, pk.xy_first))
    d = L.CocoMaskDesc()
    d.recs = recs
    d.xy, d.poly_len, d.counts = pk.xy.ctypes.data, pk.poly_len.ctypes.data, pk.counts.ctypes.data
    d.n, d.n_vert, d.n_poly, d.n_counts = n, pk.xy.shape[0], pk.poly_len.size, pk.counts.size
    lib = L.lib()
    d.ws_bytes = lib.ymi_workspace_bytes(L.WS_COCO_MASK, C.byref(d))
    ws = torch.empty(int(d.ws_bytes), dtype=torch.uint8, device=DEV)
    d.ws = ws.data_ptr()
    with torch.cuda.device(DEV):
        L.check(lib.ymi_coco_masks_u8(C.byref(d), L.stream_ptr()), 'ymi_coco_masks_u8')
        first = buf.cpu().numpy()
        buf.fill_(0xAB)
        L.check(lib.ymi_coco_masks_u8(C.byref(d), L.stream_ptr()), 'ymi_coco_masks_u8')
        second = buf.cpu().numpy()
    assert np.array_equal(first, second)                                          # two runs, equal bytes
    out, pos = [], 0
    for (h, w), o in zip(sizes, offs):
        assert (first[pos:o] == 0xAB).all(), 'guard bytes before a mask were written'
        m = first[o:o + h * w]
        assert m.max(initial=0) <= 1, 'a byte that is neither 0 nor 1 (0xAB: not written)'
        out.append(m.reshape(h, w))
        pos = o + h * w
    assert (first[pos:] == 0xAB).all(), 'guard bytes after the last mask were written'
    return out


def check(anns, sizes, want=None):
    """device == host C++ == Python oracle (== the closed form, where there is one), mask by mask."""
    got = raster(anns, sizes)
    for i, (a, (h, w)) in enumerate(zip(anns, sizes)):
        host, py = ann_to_mask(a, h, w), coco_mask.ann_to_mask(a, h, w)
        assert np.array_equal(host, py), (i, h, w, a)
        assert np.array_equal(got[i], host), (i, h, w, a, np.argwhere(got[i] != host)[:8].tolist())
        if want is not None:
            assert np.array_equal(got[i], want[i]), (i, h, w, a)
    return got


def poly(*polys):
    return {'segmentation': [list(p) for p in polys]}


def test_rectangles_have_the_closed_form_mask():
    h, w = 23, 31
    anns, want = [], []
    for (x0, y0, x1, y1) in [(2, 1, 7, 5), (0, 0, 31, 23), (30, 22, 31, 23), (5, 0, 6, 23), (0, 7, 31, 8)]:
        m = np.zeros((h, w), dtype=np.uint8)
        m[y0:y1, x0:x1] = 1
        for p in ([x0, y0, x1, y0, x1, y1, x0, y1], [x0, y0, x0, y1, x1, y1, x1, y0]):      # both orientations
            anns.append(poly(p))
            want.append(m)
    anns += [poly([40, 40, 50, 40, 50, 50]), poly([3, 3])]                                  # entirely outside; a single point
    want += [np.zeros((h, w), dtype=np.uint8)] * 2
    check(anns, [(h, w)] * len(anns), want)
    dev = ann_to_masks_device(anns, h, w, DEV)                                              # the public entry, same list
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (len(anns), h, w)
    assert np.array_equal(dev.cpu().numpy(), np.stack(want))


def test_random_polygons_match_both_restatements():
    """The generator of test_native_rasteriser_matches_the_python_restatement: integer / half-integer vertices, vertices outside
    the image, two-decimal vertices, repeated vertices; sizes 1 ... 69 (1 x 1, 1 x w, h x 1, no multiple of 32 or 64)."""
    rng = np.random.default_rng(11)
    anns, sizes = [], []
    for trial in range(300):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        k = int(rng.integers(1, 12))
        if trial % 3 == 0:
            p = (rng.integers(-6, max(h, w) + 6, 2 * k) / rng.choice([1, 2])).tolist()
        else:
            p = (rng.random(2 * k) * (max(h, w) + 10) - 5).round(2).tolist()
        if trial % 7 == 0 and k > 1:
            p[2:4] = p[0:2]
        anns.append(poly(p))
        sizes.append((h, w))
    # from the oracle: in some cases a column holds an odd number of boundary positions, so its parity carries across the
    # column end into the next column (a crossing clamped to yd = h lands on (x + 1) h) -- a per-column scan cannot pass
    carried = nonempty = 0
    for a, (h, w) in zip(anns, sizes):
        pos = np.cumsum(coco_mask.fr_poly(a['segmentation'][0], h, w))[:-1]
        per_column = np.bincount(pos // h, minlength=w + 1)[:w]
        carried += bool((per_column[:-1] % 2).any())
        nonempty += bool(len(pos))
    print('random polygons: %d non-empty, %d carry an odd parity across a column end' % (nonempty, carried))
    assert carried > 0 and nonempty > 150
    assert any(h == 1 for h, _ in sizes) and any(w == 1 for _, w in sizes) and any(h % 32 and w % 32 for h, w in sizes)
    check(anns, sizes)


def test_edge_kinds_and_borders():
    h, w = 37, 45
    anns = [
        poly([2, 2, 12, 12, 2, 12]), poly([12, 12, 2, 2, 12, 2]),               # dx == dy: the tie takes the dx >= dy branch
        poly([3.5, 3.5, 20.5, 20.5, 3.5, 30]),
        poly([1, 5, 40, 5, 40, 6, 1, 6]), poly([5, 1, 6, 1, 6, 36, 5, 36]),     # purely horizontal / vertical edges
        poly([40, 30, 10, 4, 5, 33]), poly([30, 2, 8, 30, 44, 35]),             # descending edges (flip), both slopes
        poly([30, 20, 45, 20, 45, 37, 30, 37]), poly([44, 36, 45, 36, 45, 37, 44, 37]),   # touching the last column and row
        poly([0, 36.4, 45, 36.6, 45, 50, 0, 50]), poly([44.3, 0, 60, 0, 60, 37, 44.6, 37]),
        poly([-10, -10, 60, -10, 60, 60, -10, 60]),                             # the whole image from outside
        poly([7, 7, 7, 7, 7, 7]), poly([4, 4, 4, 20]), poly([4, 9, 30, 9]),     # repeated point; degenerate two-vertex polygons
    ]
    check(anns, [(h, w)] * len(anns))
    # the smallest images, and sizes that are multiples of the bitmap's word: 1 x 1, 1 x w, h x 1, 32 x 32, 64 x 64
    sizes = [(1, 1), (1, 1), (1, 40), (1, 40), (40, 1), (40, 1), (32, 32), (64, 64), (64, 64)]
    anns = [poly([0, 0, 1, 0, 1, 1, 0, 1]), poly([0.2, 0.2, 0.4, 0.9, 0.1, 0.5]), poly([3, 0, 30, 0, 30, 1, 3, 1]), poly([-2, -2, 50, -1, 20, 4]),
            poly([0, 5, 1, 5, 1, 33, 0, 33]), poly([-2, -2, 3, 50, -1, 20]), poly([0, 0, 32, 0, 32, 32, 0, 32]),
            poly([0, 0, 64, 0, 64, 64, 0, 64]), poly([10, 63, 64, 10, 64, 64])]
    got = check(anns, sizes)
    assert got[0].all() and got[6].all() and got[7].all() and got[2].sum() == 27 and got[4].sum() == 28


UNION_A, UNION_B, UNION_C = [3, 3, 20, 4, 18, 30], [10, 10, 29, 12, 25, 39, 8, 35], [24, 2, 29, 2, 29, 8]


def test_unions():
    h, w = 40, 30
    anns = [poly(UNION_A, UNION_B), poly(UNION_A, UNION_C), poly(UNION_A, UNION_A), poly(UNION_A, UNION_B, UNION_C, UNION_A),
            poly(UNION_A), poly(UNION_B), poly(UNION_C), poly()]
    got = check(anns, [(h, w)] * len(anns))
    a, b, c = got[4], got[5], got[6]
    assert (a & b).any() and not (a & c).any()                                  # overlapping; disjoint
    assert np.array_equal(got[0], a | b) and np.array_equal(got[1], a | c)
    assert np.array_equal(got[2], a) and a.any()                                # the same polygon twice: the polygon, not empty
    assert np.array_equal(got[3], a | b | c) and not got[7].any()


def test_rle_forms():
    h, w = 40, 30
    union = ann_to_mask(poly(UNION_A, UNION_B), h, w)
    first0 = union.copy()
    first0[0, 0] = 1                                                            # the first run (of zeros) has length 0
    anns, want = [], []
    for m in (np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), first0, union):
        counts = [int(c) for c in coco_rle.rle_encode_counts(m)]
        s = coco_rle.rle_to_string(counts)
        for form in (counts, s, s.encode('ascii')):
            anns.append({'segmentation': {'size': [h, w], 'counts': form}})
            want.append(m)
    assert anns[3]['segmentation']['counts'] == [0, h * w] and anns[6]['segmentation']['counts'][0] == 0
    # zero-length runs inside: 5 zeros, 0 ones, 7 zeros, 8 ones, the rest
    anns.append({'segmentation': {'counts': [5, 0, 7, 8, h * w - 20]}})
    want.append(coco_rle.rle_decode([12, 8, h * w - 20], h, w))
    check(anns, [(h, w)] * len(anns), want)
    # many more counts than threads
    rng = np.random.default_rng(3)
    m = (rng.random((61, 67)) < 0.5).astype(np.uint8)
    counts = [int(c) for c in coco_rle.rle_encode_counts(m)]
    assert len(counts) > 1500
    check([{'segmentation': {'counts': counts}}, {'segmentation': {'counts': coco_rle.rle_to_string(counts)}}], [(61, 67)] * 2, [m, m])
    # the errors of ann_to_mask, from the public entry: exception types, and nothing half-done
    for bad, exc in (({'segmentation': {'size': [h, w], 'counts': [5, 5]}}, RuntimeError),
                     ({'segmentation': {'size': [h + 1, w], 'counts': [h * w]}}, ValueError),
                     ({'segmentation': [[1, 2, 3]]}, ValueError),
                     ({'segmentation': [[1e6, 2, 3, 4]]}, RuntimeError)):
        with pytest.raises(exc):
            ann_to_mask(bad, h, w)
        with pytest.raises(exc):
            ann_to_masks_device([anns[0], bad], h, w, DEV)


def test_one_call_with_mixed_kinds_and_two_sizes_equals_single_calls():
    m = ann_to_mask(poly(UNION_B), 40, 30)
    counts = [int(c) for c in coco_rle.rle_encode_counts(m)]
    m2 = ann_to_mask(poly([1, 1, 60, 3, 33, 20]), 21, 64)
    anns = [poly(UNION_A, UNION_B), {'segmentation': {'size': [40, 30], 'counts': counts}}, poly([1, 1, 60, 3, 33, 20], [5, 5, 9, 19, 2, 12]),
            {'segmentation': {'size': [21, 64], 'counts': coco_rle.rle_to_string(coco_rle.rle_encode_counts(m2))}}, poly(UNION_C)]
    sizes = [(40, 30), (40, 30), (21, 64), (21, 64), (40, 30)]
    together = check(anns, sizes)
    for a, s, t in zip(anns, sizes, together):
        assert np.array_equal(raster([a], [s])[0], t)
    # COCOIndex.annToMasks: each annotation at its own image's JSON size
    idx = COCOIndex()
    idx.imgs = {1: {'height': 40, 'width': 30}, 2: {'height': 21, 'width': 64}}
    for a, s in zip(anns, sizes):
        a['image_id'] = 1 if s == (40, 30) else 2
    masks = idx.annToMasks(anns, DEV)
    assert isinstance(masks, list) and all(np.array_equal(g.cpu().numpy(), t) for g, t in zip(masks, together))
    same = idx.annToMasks([anns[0], anns[1], anns[4]], DEV)
    assert torch.is_tensor(same) and tuple(same.shape) == (3, 40, 30)
    assert np.array_equal(same.cpu().numpy(), np.stack([together[0], together[1], together[4]]))


def _blob(rng, h, w, k):
    """A star-shaped polygon of k vertices somewhere in an h x w image, two-decimal coordinates as COCO's."""
    cx, cy = rng.uniform(0.2, 0.8) * w, rng.uniform(0.2, 0.8) * h
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(0.05, 0.45, k) * min(h, w)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).round(2).reshape(-1).tolist()


def test_coco_size_once_with_seven_annotations():
    h, w = 480, 640
    rng = np.random.default_rng(7)
    anns = [poly(_blob(rng, h, w, int(rng.integers(10, 81)))) for _ in range(5)]
    anns.append(poly(_blob(rng, h, w, 30), _blob(rng, h, w, 12)))
    crowd = ann_to_mask(poly(_blob(rng, h, w, 40), _blob(rng, h, w, 25)), h, w)
    anns.append({'segmentation': {'size': [h, w], 'counts': coco_rle.rle_to_string(coco_rle.rle_encode_counts(crowd))}})
    got = check(anns, [(h, w)] * 7)
    assert all(g.any() for g in got)
    assert np.array_equal(ann_to_masks_device(anns, h, w, DEV).cpu().numpy(), np.stack(got))


@pytest.mark.parametrize('h,w', [(181, 181), (128, 256), (362, 362), (256, 512), (512, 640), (800, 800)])
def test_every_kernel_size_at_its_edges(h, w):
    """The entry picks the kernel by the bitmap's words, (h w + 32) // 32 <= 1024 | 4096 | 10240 | the cap's: the largest size of
    one kernel and the smallest of the next, and the cap itself (all 160 KiB of a workgroup's LDS)."""
    rng = np.random.default_rng(h * 1000 + w)
    m = np.zeros((h, w), np.uint8)
    m[h // 3:h - 2, w // 4:w - 1] = 1
    m[h - 1, w - 1] = 1                                                          # the last pixel: the last bit of the bitmap
    anns = [poly(_blob(rng, h, w, 24), [0, 0, w, 0, w, h]), {'segmentation': {'counts': [int(c) for c in coco_rle.rle_encode_counts(m)]}}]
    got = check(anns, [(h, w)] * 2)
    assert np.array_equal(got[1], m)


def test_over_the_lds_cap_falls_back_to_the_host():
    h, w = 29, 22069                                                             # 640001 pixels: the smallest count over the cap
    assert h * w == L.COCO_MASK_MAX_PIXELS + 1
    rng = np.random.default_rng(1)
    big = poly(_blob(rng, h, w, 16), [100, 0, 9000.5, 3, 4000, 29])
    m = ann_to_mask(big, h, w)
    anns = [big, {'segmentation': {'size': [h, w], 'counts': coco_rle.rle_to_string(coco_rle.rle_encode_counts(m))}}, poly([0, 0, 50, 0, 50, 20, 0, 20])]
    d = L.CocoMaskDesc()                                                         # the entry itself refuses it ...
    pk = DC.pack_annotations(anns[:1], [(h, w)])
    rec = (L.CocoMaskRec * 1)()
    out = torch.full((h * w,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    rec[0].out, rec[0].kind, rec[0].h, rec[0].w, rec[0].n = out.data_ptr(), L.COCO_POLY, h, w, 2
    d.recs, d.xy, d.poly_len, d.n, d.n_vert, d.n_poly = rec, pk.xy.ctypes.data, pk.poly_len.ctypes.data, 1, pk.xy.shape[0], 2
    d.ws, d.ws_bytes = ws.data_ptr(), 4096
    assert L.lib().ymi_coco_masks_u8(C.byref(d), L.stream_ptr()) == L.EUNSUPPORTED
    assert bool((out == 0xAB).all()) and not bool(ws.any())
    got = ann_to_masks_device(anns, h, w, DEV)                                   # ... and the Python layer rasterises it on the host
    assert got.is_cuda and tuple(got.shape) == (3, h, w)
    got = got.cpu().numpy()
    assert m.any() and np.array_equal(got[0], m) and np.array_equal(got[1], m)
    assert np.array_equal(got[0], coco_mask.ann_to_mask(big, h, w))
    assert np.array_equal(got[2], ann_to_mask(anns[2], h, w)) and got[2].sum() == 50 * 20
    # a list that mixes sizes under and over the cap: the ones under it still go through the device call
    idx = COCOIndex()
    idx.imgs = {1: {'height': h, 'width': w}, 2: {'height': 23, 'width': 31}}
    small = dict(poly([2, 1, 7, 1, 7, 5, 2, 5]), image_id=2)
    masks = idx.annToMasks([dict(big, image_id=1), small], DEV)
    assert np.array_equal(masks[0].cpu().numpy(), m) and masks[1].cpu().numpy().sum() == 20


# ---- the pipeline --------------------------------------------------------------------------------------------------------------

def _with_max_size(S):
    yolact_amd.set_cfg('yolact_resnet50_config')
    cfg = active_cfg()
    was = cfg.max_size
    cfg.max_size = S

    def restore():
        cfg.max_size = was
    return cfg, restore


def test_pull_item_with_device_masks_equals_the_default(tmp_path):
    from yolact_amd.utils.augmentations import BaseTransform
    info = coco_synth.write_dataset(str(tmp_path))
    cfg, restore = _with_max_size(40)
    try:
        for transform in (None, BaseTransform()):
            plain = COCODetection(str(tmp_path), info, transform=transform)
            dev = COCODetection(str(tmp_path), info, transform=transform, device_masks=True)
            assert len(dev) == len(plain) == 4
            for i in range(len(plain)):
                img0, t0, m0, h0, w0, c0 = plain.pull_item(i)
                img1, t1, m1, h1, w1, c1 = dev.pull_item(i)
                assert isinstance(m0, np.ndarray) and torch.is_tensor(m1) and m1.is_cuda and m1.dtype == torch.uint8
                assert tuple(m1.shape) == m0.shape and np.array_equal(m1.cpu().numpy(), m0)
                assert np.array_equal(t0, t1) and (h0, w0, int(c0)) == (h1, w1, int(c1)) and torch.equal(img0, img1)
        # BaseTransform's discard dropped the sliver of image 139 from both
        assert dev.pull_item(0)[2].shape[0] == 3
    finally:
        restore()


def test_ssd_augmentation_batch_takes_device_masks(tmp_path):
    from yolact_amd.utils.augmentations import SSDAugmentation
    info = coco_synth.write_dataset(str(tmp_path))
    cfg, restore = _with_max_size(40)
    try:
        plain = COCODetection(str(tmp_path), info, transform=None)
        dev = COCODetection(str(tmp_path), info, transform=None, device_masks=True)
        both = []
        for ds in (plain, dev):
            items = []
            for i in range(len(ds)):
                img, target, masks, h, w, crowds = ds.pull_item(i)
                items.append((img.permute(1, 2, 0).contiguous(), masks, target[:, :4], {'num_crowds': crowds, 'labels': target[:, 4]}))
            np.random.seed(11)
            both.append(SSDAugmentation().batch(items, masks_u8=True))
        (im0, t0, m0, c0), (im1, t1, m1, c1) = both
        assert torch.equal(im0, im1) and c0 == c1 and all(torch.equal(a, b) for a, b in zip(t0, t1))
        assert len(m0) == len(m1) == 4 and all(torch.equal(a, b) for a, b in zip(m0, m1)) and any(bool(a.any()) for a in m0)
        # the single-item call, through the dataset's own transform
        np.random.seed(101)                                         # (a seed with which no item is resampled)
        a = COCODetection(str(tmp_path), info, transform=SSDAugmentation()).pull_item(1)
        np.random.seed(101)
        b = COCODetection(str(tmp_path), info, transform=SSDAugmentation(), device_masks=True).pull_item(1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and np.array_equal(a[1], b[1]) and a[5] == b[5]
    finally:
        restore()


def _add_image(ev, im, gt_masks):
    from yolact_amd.layers.box_utils import mask_bits
    cls = torch.from_numpy(im['cls']).to(DEV)
    sc = torch.from_numpy(im['score']).to(DEV)
    scores = sc if im['score2'] is None else [sc, torch.from_numpy(im['score2']).to(DEV)]
    bits = mask_bits(torch.from_numpy(im['masks'].astype(np.float32)).to(DEV))
    ev.add_detections(cls, scores, torch.from_numpy(im['box']).to(DEV), bits, im['gt'], gt_masks, im['h'], im['w'], im['num_crowd'])


def test_ap_evaluator_takes_device_masks_bit_identically():
    from yolact_amd.evaluation import APEvaluator
    meta, imgs = APR.case('crowd')
    imgs = [im for im in imgs if len(im['cls'])]
    assert imgs and any(im['num_crowd'] for im in imgs)
    host, dev = APEvaluator(meta['num_classes'], DEV), APEvaluator(meta['num_classes'], DEV)
    for im in imgs:
        gm = np.asarray(im['gt_masks'])
        _add_image(host, im, gm)
        _add_image(dev, im, torch.from_numpy(np.ascontiguousarray(gm).astype(np.uint8)).to(DEV))
    a, b = host.ap_objects(), dev.ap_objects()
    assert np.isfinite(a).any() and np.array_equal(a.view(np.uint64), b.view(np.uint64))
