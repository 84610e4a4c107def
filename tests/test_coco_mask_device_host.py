"""The device mask rasteriser's host half (no GPU): the C ABI addition (additive to ABI 9), every validation error of
ymi_coco_masks_u8 -- returned from host pointers before anything is copied or launched --, the LDS cap, the packer's tables
and the unchanged default of COCODetection.  The kernel itself: tests/test_gpu_coco_masks.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import coco_rle
from tests import coco_synth
from yolact_amd import _lib as L
from yolact_amd.data import COCODetection, ann_to_masks_device          # noqa: F401  (exported)
from yolact_amd.data import coco as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EARG, ESHAPE, ENULL, EFORMAT, EUNSUPPORTED = 0, -1, -2, -3, -4, -5


def test_abi_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, 'include', 'yolact_amd.h')).read()
    assert L.ABI_VERSION == 9 and '#define YMI_ABI_VERSION 9' in hdr and L.lib().ymi_abi_version() == 9
    sel = [(name, int(v)) for name, v in re.findall(r'\bYMI_WS_([A-Z0-9_]+) = (\d+)', hdr)]
    assert [v for _, v in sel] == list(range(1, 31)) and sel[-1] == ('COCO_MASK', 30)
    # selectors 1 ... 29 keep the names and values they had
    assert [n for n, _ in sel[:29]] == [
        'WINO_V', 'WINO_M', 'SPLITK', 'MASK_IOU', 'JPEG_COEFS', 'JPEG_PLANES', 'DETECT_SCORES_T', 'DETECT_PER_PRIOR', 'DETECT_CAND',
        'DETECT_REC', 'AMAX_SLOT', 'RLE_COUNTS', 'DETECT_GREEDY', 'JPEG_ENC', 'JPEG_ENC_OUT', 'MASK_LOSS', 'MATCH', 'BOX_LOSS',
        'CLASS_LOSS', 'SEGM_LOSS', 'MASKIOU_INPUT', 'CONV_BWD', 'MASKIOU_HEAD', 'CONV_WGRAD', 'BN', 'STEM_WGRAD', 'AUGMENT',
        'PRECONV_WGRAD', 'CONV_WGRAD_H2']
    for name, v in sel:
        assert getattr(L, 'WS_' + name) == v
    assert re.search(r'int ymi_coco_masks_u8\(const ymi_coco_mask_desc \*d, void \*stream\);', hdr)
    assert re.search(r'int64_t ymi_coco_rle_string_counts\(const char \*s, long len, uint32_t \*counts, int64_t cap\);', hdr)
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    assert bound['ymi_coco_masks_u8'] == (C.c_int, [C.POINTER(L.CocoMaskDesc), C.c_void_p])
    assert bound['ymi_coco_rle_string_counts'] == (C.c_int64, [C.c_char_p, C.c_long, C.c_void_p, C.c_int64])
    assert C.sizeof(L.CocoMaskRec) == 8 + 6 * 4 and C.sizeof(L.CocoMaskDesc) == 5 * 8 + 4 * 8 + 2 * 4
    assert '#define YMI_COCO_MASK_MAX_PIXELS %d' % L.COCO_MASK_MAX_PIXELS in hdr
    assert 'YMI_COCO_POLY = %d, YMI_COCO_COUNTS = %d' % (L.COCO_POLY, L.COCO_COUNTS) in hdr
    assert 'coco_mask.hip' in open(os.path.join(ROOT, 'yolact_amd', 'csrc', 'Makefile')).read()


class Call:
    """One valid descriptor over HOST memory (nothing may be copied or launched on an error path): a triangle and a counts
    record at 6 x 5.  `run(**changes)` applies the changes and returns the entry's code."""

    def __init__(self):
        self.h, self.w = 6, 5
        self.xy = np.array([1, 1, 4, 1, 4, 5], dtype=np.float64)
        self.poly_len = np.array([3], dtype=np.int32)
        self.counts = np.array([4, 10, 16], dtype=np.uint32)
        self.out = np.full(2 * 30 + 32, 0xAB, dtype=np.uint8)
        self.ws = np.zeros(4096 + 16, dtype=np.uint8)
        self.recs = (L.CocoMaskRec * 2)()
        base = self.out.ctypes.data
        for r, kind, n, off in ((self.recs[0], L.COCO_POLY, 1, 0), (self.recs[1], L.COCO_COUNTS, 3, 30)):
            r.out, r.kind, r.h, r.w, r.n, r.first, r.xy_first = base + off, kind, self.h, self.w, n, 0, 0
        d = self.d = L.CocoMaskDesc()
        d.recs = self.recs
        d.xy, d.poly_len, d.counts = self.xy.ctypes.data, self.poly_len.ctypes.data, self.counts.ctypes.data
        d.n, d.n_vert, d.n_poly, d.n_counts = 2, 3, 1, 3
        d.ws = (self.ws.ctypes.data + 15) // 16 * 16
        d.ws_bytes = 4096

    def run(self):
        rc = L.lib().ymi_coco_masks_u8(C.byref(self.d), None)
        assert (self.out == 0xAB).all() and not self.ws.any()          # an error path writes nothing
        return rc


def test_workspace_selector():
    c = Call()
    need = L.lib().ymi_workspace_bytes(L.WS_COCO_MASK, C.byref(c.d))
    assert need == 48 + 64 + 16 + 16            # 3 vertices of 16 bytes | 2 records of 32 | 1 length | 3 counts, each padded to 16
    c.d.n = 0
    assert L.lib().ymi_workspace_bytes(L.WS_COCO_MASK, C.byref(c.d)) < 0


def test_every_validation_error_is_returned_before_a_launch():
    lib = L.lib()
    assert lib.ymi_coco_masks_u8(None, None) == ENULL

    def expect(code, change):
        c = Call()
        change(c)
        assert c.run() == code, (code, change)

    def setd(**kw):
        return lambda c: [setattr(c.d, k, v) for k, v in kw.items()]

    def setr(i, **kw):
        return lambda c: [setattr(c.recs[i], k, v) for k, v in kw.items()]

    # NULL pointers
    expect(ENULL, setd(recs=C.POINTER(L.CocoMaskRec)()))
    expect(ENULL, setd(ws=None))
    expect(ENULL, setd(xy=None))
    expect(ENULL, setd(poly_len=None))
    expect(ENULL, setd(counts=None))
    expect(ENULL, setr(0, out=None))
    expect(ENULL, setr(1, out=None))
    # arguments
    expect(EARG, setd(n=0))
    expect(EARG, lambda c: c.poly_len.__setitem__(0, 0))                  # k < 1
    for i in (0, 1):
        expect(EARG, setr(i, h=0))
        expect(EARG, setr(i, w=-3))
        expect(EARG, setr(i, n=-1))
    expect(EARG, setr(0, kind=2))
    lim = 3 * 6 + 1024                                                    # |coordinate| <= 3 max(w, h) + 1024
    for j, v in ((0, lim + 1.0), (3, -(lim + 1.0)), (5, float('nan')), (2, float('inf'))):
        expect(EARG, lambda c, j=j, v=v: c.xy.__setitem__(j, v))
    # counts
    expect(EFORMAT, lambda c: c.counts.__setitem__(2, 15))                # do not sum to h w
    expect(EFORMAT, lambda c: c.counts.__setitem__(1, 27))                # a run past the end
    expect(EFORMAT, setr(1, n=2))
    expect(EFORMAT, setr(1, n=0))
    # the records' ranges and the workspace
    expect(ESHAPE, setr(0, first=1))
    expect(ESHAPE, setr(0, xy_first=1))
    expect(ESHAPE, setr(0, xy_first=-1))
    expect(ESHAPE, setr(1, first=1))
    expect(ESHAPE, setd(n_vert=2))
    expect(ESHAPE, setd(ws_bytes=143))
    expect(ESHAPE, lambda c: setattr(c.d, 'ws', c.d.ws + 8))
    # an error in a later record is found although the first is fine; the first error wins
    expect(EARG, lambda c: (setr(1, h=0)(c), setd(ws_bytes=0)(c)))


def test_over_the_lds_cap_is_unsupported_and_the_cap_is_tight():
    cap = L.COCO_MASK_MAX_PIXELS
    assert cap == 640000 and (2 * ((cap + 32) // 32) + 16) * 4 <= 160 * 1024      # two bitmaps of cap + 1 bits and the scan scratch
    for h, w in ((801, 800), (1, cap + 1), (cap + 1, 1)):
        c = Call()
        c.recs[0].h, c.recs[0].w = h, w
        assert c.run() == EUNSUPPORTED, (h, w)
        c = Call()                                                                # a counts record over the cap, valid counts
        c.recs[1].h, c.recs[1].w = h, w
        c.counts[:] = (4, 10, h * w - 14)
        assert c.run() == EUNSUPPORTED, (h, w)
    c = Call()                                                                    # over the cap AND bad counts: the counts' code
    c.recs[1].h, c.recs[1].w = 801, 800
    assert c.run() == EFORMAT


def test_string_counts_are_the_oracles():
    rng = np.random.default_rng(5)
    for trial in range(40):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        m = (rng.random((h, w)) < rng.random()).astype(np.uint8)
        counts = coco_rle.rle_encode_counts(m)
        s = coco_rle.rle_to_string(counts)
        for form in (s, s.encode('ascii')):
            got = DC.string_counts(form)
            assert got.dtype == np.uint32 and got.tolist() == [int(c) for c in coco_rle.rle_from_string(s)] == [int(c) for c in counts]
    assert DC.string_counts('').size == 0
    with pytest.raises(RuntimeError):
        DC.string_counts('o')                                      # a continuation bit and then the end of the string
    # the host fill still decodes the same way (the code is shared)
    m = np.zeros((7, 9), dtype=np.uint8)
    m[2:5, 3:8] = 1
    s = coco_rle.rle_to_string(coco_rle.rle_encode_counts(m))
    assert np.array_equal(DC.ann_to_mask({'segmentation': {'size': [7, 9], 'counts': s}}, 7, 9), m)


def test_packer_tables_for_a_mixed_list():
    m = np.zeros((12, 9), dtype=np.uint8)
    m[3:8, 2:7] = 1
    counts = [int(c) for c in coco_rle.rle_encode_counts(m)]
    s = coco_rle.rle_to_string(counts)
    tri, quad, pt = [1, 1, 8, 2, 4, 9.5], [0, 0, 9, 0, 9, 12, 0, 12], [3, 3]
    anns = [{'segmentation': [tri, quad]},
            {'segmentation': {'size': [12, 9], 'counts': counts}},
            {'segmentation': []},
            {'segmentation': {'counts': s}},
            {'segmentation': [pt]},
            {'segmentation': {'size': [20, 4], 'counts': s.encode('ascii')}}]
    sizes = [(12, 9)] * 5 + [(20, 4)]
    pk = DC.pack_annotations(anns, sizes)
    assert len(pk) == 6
    for a in (pk.kind, pk.h, pk.w, pk.n, pk.first, pk.xy_first, pk.poly_len):
        assert a.dtype == np.int32
    assert pk.kind.tolist() == [L.COCO_POLY, L.COCO_COUNTS, L.COCO_POLY, L.COCO_COUNTS, L.COCO_POLY, L.COCO_COUNTS]
    assert pk.h.tolist() == [12] * 5 + [20] and pk.w.tolist() == [9] * 5 + [4]
    nc = len(counts)
    assert pk.n.tolist() == [2, nc, 0, nc, 1, nc]
    assert pk.first.tolist() == [0, 0, 2, nc, 2, 2 * nc]
    assert pk.xy_first.tolist() == [0, 0, 7, 0, 7, 0]
    assert pk.poly_len.tolist() == [3, 4, 1]
    assert pk.xy.dtype == np.float64 and pk.xy.shape == (8, 2) and pk.xy.reshape(-1).tolist() == [float(v) for v in tri + quad + pt]
    assert pk.counts.dtype == np.uint32 and pk.counts.tolist() == counts + [int(c) for c in coco_rle.rle_from_string(s)] * 2
    # the shape errors of ann_to_mask, with its exception types
    for bad in ({'segmentation': [[1, 2, 3]]}, {'segmentation': [[1]]}, {'segmentation': [tri, []]},
                {'segmentation': {'size': [13, 9], 'counts': counts}}):
        with pytest.raises(ValueError):
            DC.pack_annotations([anns[0], bad], [(12, 9)] * 2)
        with pytest.raises(ValueError):
            DC.ann_to_mask(bad, 12, 9)
    with pytest.raises(RuntimeError):
        DC.pack_annotations([{'segmentation': {'counts': 'o'}}], [(12, 9)])
    empty = DC.pack_annotations([], [])
    assert len(empty) == 0 and empty.xy.shape == (0, 2) and empty.counts.size == 0 and empty.poly_len.size == 0


def test_default_dataset_still_returns_numpy_masks(tmp_path, monkeypatch):
    import inspect
    import torch
    from oracle import coco_mask
    assert inspect.signature(COCODetection.__init__).parameters['device_masks'].default is False
    ds = COCODetection(str(tmp_path), coco_synth.write_dataset(str(tmp_path)))
    assert ds.device_masks is False
    # the image decode is the GPU's: stand in a host tensor of the JSON size, the annotation half is what is under test
    sizes = {i['file_name'].split('_')[-1]: (i['height'], i['width']) for i in ds.coco.imgs.values()}
    monkeypatch.setattr(DC.jpeg, 'imread', lambda path, device=None: torch.zeros(sizes[os.path.basename(path)] + (3,), dtype=torch.uint8))
    monkeypatch.setattr(ds.coco, 'annToMasks', None)                     # the default route never asks for device masks
    for index, img_id in enumerate(ds.ids):
        if img_id == 632:
            continue                                                     # (decodes rotated: the stand-in has no EXIF)
        img, target, masks, h, w, num_crowds = ds.pull_item(index)
        anns, nc = DC._split_crowds([dict(a) for a in ds.coco.loadAnns(ds.coco.getAnnIds(imgIds=img_id))])
        assert isinstance(masks, np.ndarray) and masks.dtype == np.uint8 and masks.shape == (len(anns), h, w) and num_crowds == nc
        for m, a in zip(masks, anns):
            assert np.array_equal(m, coco_mask.ann_to_mask(a, h, w))
