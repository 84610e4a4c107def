"""The image write of evalimage / evalimages / evalvideo (eval.py: `cv2.imwrite(save_path, img_numpy)`), CPU half.

cv2.imwrite of a .jpg = libjpeg with its defaults.  tests/golden/jpeg_encode.npz holds, per case, input pixels and the bytes
libjpeg-turbo wrote for them through Pillow (tools/make_golden_jpeg_encode.py): sizes 1x1 .. 100x75 with odd block counts
(dummy blocks), noise / gradient / all-0 / all-255 / 0-255 checkerboard / a composited-looking frame, qualities
1, 50, 75, 95, 100 in 4:2:0 and 4:4:4, and two photo-sized frames as SHA-256 + length.  The bar is BYTE EQUALITY of the file.

CPU (this file, no GPU):
  * the DEVICE arithmetic executed on the host: tests/jpeg_enc_emul.cpp (built here with g++) loops over the scan's blocks
    calling the very inline functions the kernels call (csrc/jpeg_enc_math.h) -> bytes equal to every golden, and to Pillow live;
  * the product's host half through the C ABI: ymi_jpeg_write_header == the golden's bytes up to and including SOS, the
    quantisation tables, the new symbols and workspace selectors at ABI 9, the documented error codes, the output bound;
  * the produced files through the project's own decoder (ymi_jpeg_parse + ymi_jpeg_decode_coefs): the emulation's own
    coefficients and tables come back.
GPU: tests/test_gpu_jpeg_encode.py runs the kernels themselves through ymi_jpeg_encode_bgr_u8 on the same cases.
"""
import ctypes as C
import hashlib
import io
import os
import subprocess

import numpy as np
import pytest

from tests import jpeg_enc_cases as K
from yolact_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, 'golden', 'jpeg_encode.npz'))
CASES = K.cases()
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def build_emul(directory):
    so = os.path.join(str(directory), 'libjpeg_enc_emul.so')
    subprocess.run(['g++', '-O2', '-shared', '-fPIC', '-o', so, os.path.join(HERE, 'jpeg_enc_emul.cpp')], check=True)
    lib = C.CDLL(so)
    lib.emul_jpeg_encode_bgr_u8.restype = C.c_int64
    lib.emul_jpeg_encode_bgr_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                            C.c_void_p]
    return lib


def header(h, w, quality, sub):
    buf = np.zeros(L.JPEG_HEADER_BYTES, np.uint8)
    n = C.c_size_t()
    L.check(L.lib().ymi_jpeg_write_header(h, w, quality, sub, buf.ctypes.data, buf.size, C.byref(n)), 'ymi_jpeg_write_header')
    return buf[:n.value].tobytes()


def out_bound(h, w, sub):
    d = L.JpegEncDesc(h=h, w=w, quality=95, subsampling=sub)
    return L.lib().ymi_workspace_bytes(L.WS_JPEG_ENC_OUT, C.byref(d))


def n_blocks(h, w, sub):
    m = 16 if sub == 2 else 8
    return -(-h // m) * -(-w // m) * (6 if sub == 2 else 3)


def emul_encode(emul, bgr, quality, sub, want_coefs=False):
    """The file the device path must write, from the host emulation of its arithmetic (+ its coefficients)."""
    h, w = bgr.shape[:2]
    assert bgr.dtype == np.uint8 and bgr.strides[2] == 1 and bgr.strides[1] == 3
    cap = out_bound(h, w, sub)
    out = np.zeros(cap, np.uint8)
    coefs = np.zeros(n_blocks(h, w, sub) * 64, np.int16)
    n = emul.emul_jpeg_encode_bgr_u8(bgr.ctypes.data, h, w, bgr.strides[0], quality, sub, out.ctypes.data, cap, coefs.ctypes.data)
    assert n > 0, n
    data = header(h, w, quality, sub) + out[:n].tobytes()
    return (data, coefs) if want_coefs else data


def pillow_encode(bgr, quality, sub):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, 'JPEG', quality=quality, subsampling=sub)
    return buf.getvalue()


def gold(case):
    name, content, h, w, q, s = case
    px = GOLD['px_%dx%d_%s' % (h, w, content)]
    assert np.array_equal(px, K.pixels(content, h, w)), name      # the generator still makes the stored pixels
    return np.ascontiguousarray(px), GOLD['jpg_' + name].tobytes()


@pytest.fixture(scope='module')
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp('enc_emul'))


def test_fixture_inventory():
    assert len(CASES) == 9 * 6 + 3 * 3 * 9 and len({c[0] for c in CASES}) == len(CASES)
    assert all('jpg_' + c[0] in GOLD.files for c in CASES)
    assert {(c[2], c[3]) for c in CASES} == set(K.SIZES)
    assert {(c[4], c[5]) for c in CASES} == {(q, s) for q in K.QUALITIES for s in K.SUBS}
    assert 'libjpeg-turbo' in str(GOLD['versions'][1])
    for h, w, _ in K.LARGE:
        assert GOLD['big_%dx%d_sha256' % (h, w)].size == 32 and int(GOLD['big_%dx%d_len' % (h, w)]) > 1000


def test_golden_files_have_the_fixed_layout():
    """SOI, APP0 (JFIF 1.01, density 1:1), DQT, DQT, SOF0, DHT x 4, SOS: what the issue fixes, checked on libjpeg's own bytes."""
    for case in CASES:
        _, data = gold(case)
        p, markers = 2, []
        while True:
            assert data[p] == 0xFF
            markers.append(data[p + 1])
            p += 2 + int.from_bytes(data[p + 2:p + 4], 'big')
            if markers[-1] == 0xDA:
                break
        assert data[:2] == b'\xff\xd8' and markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA], case[0]
        assert p == L.JPEG_HEADER_BYTES and data[-2:] == b'\xff\xd9'
        assert data[4:20] == b'\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'


def test_emulation_bytes_equal_every_golden(emul):
    bad = []
    for case in CASES:
        px, want = gold(case)
        got = emul_encode(emul, px, case[4], K.SUBS[case[5]])
        if got != want:
            bad.append((case[0], len(got), len(want)))
    assert not bad, bad[:10]


def test_emulation_equals_golden_digest_on_photo_sized_frames(emul):
    for h, w, seed in K.LARGE:
        got = emul_encode(emul, K.frame(h, w, seed), 95, 2)
        assert len(got) == int(GOLD['big_%dx%d_len' % (h, w)])
        assert hashlib.sha256(got).digest() == GOLD['big_%dx%d_sha256' % (h, w)].tobytes()


def test_emulation_bytes_equal_pillow_live(emul):
    pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(21)
    shapes = [(1, 1), (1, 40), (40, 1), (2, 2), (9, 23), (16, 32), (18, 34), (31, 17), (33, 47), (48, 80), (129, 65)]
    for i, (h, w) in enumerate(shapes):
        q = int(rng.integers(1, 101))
        for px in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), K.frame(h, w, 100 + i)):
            for sub in (2, 0):
                assert emul_encode(emul, px, q, sub) == pillow_encode(px, q, sub), (h, w, q, sub)
    # an arbitrary row stride: a window of a larger frame
    big = rng.integers(0, 256, (40, 70, 3), dtype=np.uint8)
    win = big[3:36, 5:52]
    assert emul_encode(emul, win, 95, 2) == pillow_encode(win, 95, 2)


def test_header_equals_golden_up_to_sos():
    for case in CASES:
        _, data = gold(case)
        got = header(case[2], case[3], case[4], K.SUBS[case[5]])
        assert len(got) == L.JPEG_HEADER_BYTES and got == data[:L.JPEG_HEADER_BYTES], case[0]


def test_quantisation_tables_are_the_headers():
    lib = L.lib()
    for q in (1, 2, 25, 49, 50, 51, 75, 95, 99, 100):
        qt = np.zeros(128, np.uint16)
        assert lib.ymi_jpeg_enc_qtables(q, qt.ctypes.data) == 0
        hdr = header(8, 8, q, 2)
        i = hdr.index(b'\xff\xdb')
        for t in range(2):
            seg = hdr[i + 69 * t:i + 69 * (t + 1)]
            assert seg[:5] == b'\xff\xdb\x00\x43' + bytes([t])
            assert [int(qt[64 * t + ZIGZAG[k]]) for k in range(64)] == list(seg[5:]), (q, t)
        assert qt.min() >= 1 and qt.max() <= 255
    qt = np.zeros(128, np.uint16)
    lib.ymi_jpeg_enc_qtables(95, qt.ctypes.data)
    assert list(qt[[0, 1, 8, 16]]) == [2, 1, 1, 1]          # DQT[0..3] in zigzag order at quality 95
    lib.ymi_jpeg_enc_qtables(100, qt.ctypes.data)
    assert (qt == 1).all()
    assert lib.ymi_jpeg_enc_qtables(0, qt.ctypes.data) == -1 and lib.ymi_jpeg_enc_qtables(50, None) == -3


def test_new_entries_exist_at_abi_9():
    lib = L.lib()
    assert lib.ymi_abi_version() == 9 and L.ABI_VERSION == 9
    for sym in ('ymi_jpeg_write_header', 'ymi_jpeg_enc_qtables', 'ymi_jpeg_encode_bgr_u8'):
        assert hasattr(lib, sym) and sym in {s for s, _, _ in L.SYMBOLS}
    assert (L.WS_JPEG_ENC, L.WS_JPEG_ENC_OUT) == (14, 15) and L.WS_DETECT_GREEDY == 13
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'yolact_amd.h')).read()
    assert 'YMI_WS_JPEG_ENC = 14' in hdr and 'YMI_WS_JPEG_ENC_OUT = 15' in hdr and '#define YMI_ABI_VERSION 9' in hdr
    assert C.sizeof(L.JpegEncDesc) == 8 + 2 * 4 + 8 + 2 * 4 + 8 + 8 + 8 + 8
    d = L.JpegEncDesc(h=550, w=550, quality=95, subsampling=2)
    assert lib.ymi_workspace_bytes(L.WS_JPEG_ENC, C.byref(d)) > 35 * 35 * 6 * 128
    assert lib.ymi_workspace_bytes(L.WS_JPEG_ENC_OUT, C.byref(d)) == 35 * 35 * 6 * 416 + 2


def test_argument_errors():
    lib = L.lib()
    buf = np.zeros(1024, np.uint8)
    n = C.c_size_t()
    ok = lambda *a: lib.ymi_jpeg_write_header(*a, buf.ctypes.data, buf.size, C.byref(n))       # noqa: E731
    assert ok(1, 1, 1, 0) == 0 and ok(65535, 65535, 100, 2) == 0
    for bad in ((0, 8, 95, 2), (8, 0, 95, 2), (65536, 8, 95, 2), (8, 65536, 95, 2), (8, 8, 0, 2), (8, 8, 101, 2), (8, 8, 95, 1),
                (8, 8, 95, 3), (-1, 8, 95, 2)):
        assert ok(*bad) == -1, bad
    assert lib.ymi_jpeg_write_header(8, 8, 95, 2, buf.ctypes.data, 100, C.byref(n)) == -1        # capacity
    assert lib.ymi_jpeg_write_header(8, 8, 95, 2, None, 1024, C.byref(n)) == -3
    assert lib.ymi_jpeg_write_header(8, 8, 95, 2, buf.ctypes.data, 1024, None) == -3
    for what in (L.WS_JPEG_ENC, L.WS_JPEG_ENC_OUT):
        assert lib.ymi_workspace_bytes(what, None) == -3
        for h, w, s in ((0, 8, 2), (8, 65536, 2), (8, 8, 1)):
            d = L.JpegEncDesc(h=h, w=w, quality=95, subsampling=s)
            assert lib.ymi_workspace_bytes(what, C.byref(d)) == -1
    # the device entry validates BEFORE it touches the GPU: these return without a launch (pointers are never dereferenced)
    fake = 1 << 20
    good = dict(img=fake, h=16, w=16, row_stride=48, quality=95, subsampling=2, out=fake, out_capacity=out_bound(16, 16, 2),
                out_len=fake, ws=fake)
    assert lib.ymi_jpeg_encode_bgr_u8(None, None) == -3
    for k in ('img', 'out', 'out_len', 'ws'):
        assert lib.ymi_jpeg_encode_bgr_u8(C.byref(L.JpegEncDesc(**dict(good, **{k: None}))), None) == -3, k
    for k, v in (('h', 0), ('w', 65536), ('quality', 0), ('quality', 101), ('subsampling', 1), ('row_stride', 47),
                 ('out_capacity', out_bound(16, 16, 2) - 1), ('out_capacity', 0)):
        assert lib.ymi_jpeg_encode_bgr_u8(C.byref(L.JpegEncDesc(**dict(good, **{k: v}))), None) == -1, (k, v)


def test_out_bound_covers_every_golden_scan(emul):
    for case in CASES:
        _, data = gold(case)
        sub = K.SUBS[case[5]]
        bound = out_bound(case[2], case[3], sub)
        assert bound == 416 * n_blocks(case[2], case[3], sub) + 2
        assert bound >= len(data) - L.JPEG_HEADER_BYTES, case[0]
    # the worst stream a baseline coder can be driven to is still inside it: checkerboard and noise at quality 100, 4:4:4
    for content in ('checker', 'noise'):
        px = K.pixels(content, 64, 48)
        assert len(emul_encode(emul, px, 100, 0)) - L.JPEG_HEADER_BYTES <= out_bound(64, 48, 0)


def test_own_decoder_returns_the_emulations_coefficients(emul):
    """ymi_jpeg_parse + ymi_jpeg_decode_coefs on the produced bytes: sizes, sampling, tables and every coefficient."""
    lib = L.lib()
    for case in CASES:
        px, _ = gold(case)
        h, w, q, sub = case[2], case[3], case[4], K.SUBS[case[5]]
        data, zz = emul_encode(emul, px, q, sub, want_coefs=True)
        info = L.JpegInfo()
        L.check(lib.ymi_jpeg_parse(data, len(data), C.byref(info)), 'ymi_jpeg_parse')
        assert (info.height, info.width, info.ncomp, info.progressive) == (h, w, 3, 0), case[0]
        assert (info.hs[0], info.vs[0]) == ((2, 2) if sub == 2 else (1, 1)) and (info.hs[1], info.vs[2]) == (1, 1)
        coefs = np.full(int(info.coef_count), 12345, np.int16)
        qt = np.zeros(192, np.uint16)
        L.check(lib.ymi_jpeg_decode_coefs(data, len(data), coefs.ctypes.data, coefs.size, qt.ctypes.data, C.byref(info)),
                'ymi_jpeg_decode_coefs')
        want_qt = np.zeros(128, np.uint16)
        lib.ymi_jpeg_enc_qtables(q, want_qt.ctypes.data)
        assert np.array_equal(qt[:64], want_qt[:64]) and np.array_equal(qt[64:128], want_qt[64:]) and np.array_equal(
            qt[128:], want_qt[64:]), case[0]
        # emulation: scan order [mcu][block][zigzag]; decoder: [component][by][bx][natural]
        m = 2 if sub == 2 else 1
        mcuy, mcux = -(-h // (8 * m)), -(-w // (8 * m))
        zz = zz.reshape(mcuy, mcux, m * m + 2, 64)
        nat = np.zeros_like(zz)
        nat[..., ZIGZAG] = zz
        luma = nat[:, :, :m * m].reshape(mcuy, mcux, m, m, 64).transpose(0, 2, 1, 3, 4).reshape(-1)
        want = np.concatenate([luma, nat[:, :, m * m].reshape(-1), nat[:, :, m * m + 1].reshape(-1)])
        assert coefs.size == want.size and np.array_equal(coefs, want), case[0]


def test_python_entries_refuse_cpu_tensors():
    import torch
    from yolact_amd.data import jpeg
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        jpeg.imencode(img)
    with pytest.raises(RuntimeError):
        jpeg.imwrite('/nonexistent/x.jpg', img)
    assert jpeg.write_header(16, 16, 95, '4:2:0') == header(16, 16, 95, 2)
    with pytest.raises(ValueError):
        jpeg.write_header(16, 16, 0)
    with pytest.raises(ValueError):
        jpeg.write_header(16, 16, 95, '4:2:2')
