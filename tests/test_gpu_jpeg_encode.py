"""GPU: the image write of evalimage / evalimages / evalvideo (eval.py: `cv2.imwrite(save_path, img_numpy)`) through
ymi_jpeg_encode_bgr_u8 — `yolact_amd.data.jpeg.imencode / imwrite / JpegEncoder`.

Every expected value comes from libjpeg-turbo's own bytes (tests/golden/jpeg_encode.npz, written through Pillow) or from the host
emulation of the device arithmetic (tests/jpeg_enc_emul.cpp, itself pinned to the goldens by tests/test_jpeg_encode.py), never
from the kernels under test.  The bar is byte equality of the whole file.
"""
import hashlib
import io

import numpy as np
import pytest
import torch

from tests import jpeg_enc_cases as K
from tests import test_jpeg_encode as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    return T.build_emul(tmp_path_factory.mktemp('enc_emul_gpu'))


def test_imencode_bytes_equal_every_golden():
    from yolact_amd.data import jpeg
    bad = []
    for case in T.CASES:
        px, want = T.gold(case)
        got = jpeg.imencode(torch.from_numpy(px).to(DEV), quality=case[4], subsampling={'420': '4:2:0', '444': '4:4:4'}[case[5]])
        if got != want:
            bad.append((case[0], len(got), len(want)))
    assert not bad, bad[:10]


def test_photo_sized_frames_match_the_golden_digest():
    from yolact_amd.data import jpeg
    for h, w, seed in K.LARGE:
        got = jpeg.imencode(torch.from_numpy(K.frame(h, w, seed)).to(DEV))
        assert len(got) == int(T.GOLD['big_%dx%d_len' % (h, w)]), (h, w)
        assert hashlib.sha256(got).digest() == T.GOLD['big_%dx%d_sha256' % (h, w)].tobytes(), (h, w)


def test_random_sizes_and_row_strides_equal_the_host_emulation(emul):
    from yolact_amd.data import jpeg
    rng = np.random.default_rng(33)
    shapes = [(1, 1), (1, 77), (93, 1), (2, 3), (24, 40), (123, 211), (250, 97), (301, 303)]
    for i, (h, w) in enumerate(shapes):
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if i % 2 == 0 else K.frame(h, w, 200 + i)
        q = int(rng.integers(1, 101))
        for sub, name in ((2, '4:2:0'), (0, '4:4:4')):
            assert jpeg.imencode(torch.from_numpy(px).to(DEV), q, name) == T.emul_encode(emul, px, q, sub), (h, w, q, name)
    # a window of a larger frame: row stride > 3 * w and a start that is not 16-byte aligned; no copy is made
    big = rng.integers(0, 256, (140, 200, 3), dtype=np.uint8)
    win = torch.from_numpy(big).to(DEV)[7:130, 5:170]
    assert not win.is_contiguous() and win.stride(0) == 600
    assert jpeg.imencode(win, 90) == T.emul_encode(emul, np.ascontiguousarray(big[7:130, 5:170]), 90, 2)
    # noise at quality 100, 4:4:4: a stream longer than the encoder's first read-back guess (the second transfer)
    px = rng.integers(0, 256, (96, 160, 3), dtype=np.uint8)
    want = T.emul_encode(emul, px, 100, 0)
    assert len(want) > 96 * 160 * 3 // 4 + 623
    assert jpeg.imencode(torch.from_numpy(px).to(DEV), 100, '4:4:4') == want


def test_encode_many_equals_single_encodes(emul):
    from yolact_amd.data import jpeg
    h, w = 120, 176
    frames = [K.frame(h, w, 300 + i) if i % 3 else K.pixels('noise', h, w, 300 + i) for i in range(8)]
    dev = [torch.from_numpy(f).to(DEV) for f in frames]
    enc = jpeg.JpegEncoder(h, w, 95, '4:2:0', DEV)
    many = enc.encode_many(dev)
    assert len(many) == 8 and len(set(many)) == 8
    assert many == [enc.encode(f) for f in dev]
    assert many == [T.emul_encode(emul, f, 95, 2) for f in frames]
    # a fresh encoder whose guess is too small for the noise frames: the re-encode path gives the same files
    enc2 = jpeg.JpegEncoder(h, w, 95, '4:2:0', DEV)
    enc2.guess = 1024
    assert enc2.encode_many(dev) == many


def test_imwrite_then_imread_decodes_to_libjpeg_turbos_pixels(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from yolact_amd.data import jpeg
    for name in ('37x53_frame_q95_420', '100x75_noise_q95_420', '17x33_checker_q50_444'):
        case = next(c for c in T.CASES if c[0] == name)
        px, want = T.gold(case)
        path = str(tmp_path / (name + '.jpg'))
        assert jpeg.imwrite(path, torch.from_numpy(px).to(DEV), case[4], {'420': '4:2:0', '444': '4:4:4'}[case[5]]) is True
        assert open(path, 'rb').read() == want
        ref = np.array(Image.open(io.BytesIO(want)).convert('RGB'))[..., ::-1]      # libjpeg-turbo's decode of the GOLDEN bytes
        got = jpeg.imread(path)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref), name


def test_prep_display_frame_encodes_like_the_host_emulation(emul):
    """imread-style frame -> network -> prep_display -> imencode on r50_dense: the file equals the emulation's for that frame."""
    import yolact_amd
    from helpers import case_images, oracle_run
    from gpu_utils import build_net
    from yolact_amd import display
    from yolact_amd.data import jpeg
    meta, arrays, cfg, sd, raw, dets = oracle_run('r50_dense')
    yolact_amd.set_cfg(meta['config'])
    net = build_net(meta, DEV)
    preds = net(case_images(meta).to(DEV))
    frame = torch.from_numpy(K.frame(480, 640, 77)).to(DEV).float()
    shown = display.prep_display(preds, frame, top_k=5)[0]
    assert shown.dtype == torch.uint8 and tuple(shown.shape) == (480, 640, 3) and shown.is_cuda
    assert not torch.equal(shown, frame.to(torch.uint8))           # masks were composited
    got = jpeg.imencode(shown)
    assert got == T.emul_encode(emul, np.ascontiguousarray(shown.cpu().numpy()), 95, 2)


def test_argument_errors_raise():
    from yolact_amd.data import jpeg
    img = torch.zeros(16, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        jpeg.imencode(img.cpu())
    with pytest.raises(ValueError):
        jpeg.imencode(img, quality=0)
    with pytest.raises(ValueError):
        jpeg.imencode(img, quality=101)
    with pytest.raises(ValueError):
        jpeg.imencode(img, subsampling='4:2:2')
    with pytest.raises(ValueError):
        jpeg.imencode(img.float())
    with pytest.raises(ValueError):
        jpeg.imencode(img[..., :2])
    with pytest.raises(ValueError):
        jpeg.imencode(img[0])
    with pytest.raises(TypeError):
        jpeg.imencode(np.zeros((16, 16, 3), np.uint8))
    with pytest.raises(ValueError):
        jpeg.JpegEncoder(16, 16, 95, '4:2:0', DEV).encode(torch.zeros(8, 16, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        jpeg.JpegEncoder(0, 16)
    # the C entry: a capacity below the bound is refused at call time
    import ctypes as C
    from yolact_amd import _lib as L
    enc = jpeg.JpegEncoder(16, 16, 95, '4:2:0', DEV)
    d = L.JpegEncDesc(img=img.data_ptr(), h=16, w=16, row_stride=48, quality=95, subsampling=2, out=enc.out.data_ptr() + 8,
                      out_capacity=enc.cap - 1, out_len=enc.out.data_ptr(), ws=enc.ws.data_ptr())
    assert L.lib().ymi_jpeg_encode_bgr_u8(C.byref(d), L.stream_ptr()) == -1
