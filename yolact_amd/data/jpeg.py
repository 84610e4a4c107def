"""`cv2.imread` for JPEG files with the pixel work on the GPU (COCODetection.pull_item, data/coco.py:138-141).

cv2.imread(path) on a JPEG = libjpeg-turbo with its defaults + EXIF orientation -> uint8 BGR [h,w,3].  Here the serial
half (markers, Huffman decoding; csrc/jpeg_host.cpp) runs on the host and hands the quantised coefficient blocks to the
GPU, which does everything data parallel (dequantise, ISLOW IDCT, fancy chroma upsampling, YCbCr -> BGR, orientation;
csrc/jpeg.hip).  The result is bit-identical to libjpeg-turbo's (tests/test_jpeg.py, tests/test_gpu_jpeg.py) and stays
on the device for the transform that follows.  Not a JPEG -> ValueError (cv2 would try its other codecs; COCO is JPEG
only); corrupt / unsupported streams -> RuntimeError with the library's message.  There is no CPU decode path.

`imencode` / `imwrite` / `JpegEncoder` are the write side: eval.py's `cv2.imwrite(save_path, img_numpy)` for a frame that is
already on the device (display.prep_display).  The whole encoder runs on the GPU (csrc/jpeg_enc.hip); the host writes the
623-byte header and reads the finished stream back.  Byte-equal to libjpeg-turbo's output through Pillow at the same quality
and subsampling (tests/test_jpeg_encode.py, tests/test_gpu_jpeg_encode.py).  There is no CPU encode path.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

from .. import _lib as L


MAX_COEFS = 1 << 29        # 512 M coefficients (a 16k x 16k 4:4:4 image); a corrupt header must not allocate 26 GB


class JpegInfo:
    """Plain-Python view of ymi_jpeg_info."""

    def __init__(self, raw: L.JpegInfo):
        self.raw = raw
        self.width, self.height = raw.width, raw.height
        self.out_width, self.out_height = raw.out_width, raw.out_height
        self.ncomp, self.progressive, self.orientation, self.color = raw.ncomp, bool(raw.progressive), raw.orientation, raw.color
        self.sampling = [(raw.hs[i], raw.vs[i]) for i in range(raw.ncomp)]
        self.coef_count, self.plane_bytes = raw.coef_count, raw.plane_bytes


def _as_bytes(src) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    if isinstance(src, (str, os.PathLike)):
        with open(src, 'rb') as f:
            return f.read()
    raise TypeError('imread: a path or the file bytes, got %r' % type(src))


def parse(src) -> JpegInfo:
    """Header only (host): sizes, sampling, progressive flag, EXIF orientation."""
    data = _as_bytes(src)
    if data[:2] != b'\xff\xd8':
        raise ValueError('not a JPEG stream (no SOI marker)')
    raw = L.JpegInfo()
    L.check(L.lib().ymi_jpeg_parse(data, len(data), C.byref(raw)), 'ymi_jpeg_parse')
    if raw.coef_count > MAX_COEFS:
        raise ValueError('JPEG header declares %d x %d pixels: larger than this reader accepts' % (raw.width, raw.height))
    return JpegInfo(raw)


class _Staging(threading.local):
    """Per-thread pinned staging buffer for the coefficients (grown on demand); the event orders its reuse behind the
    previous image's host-to-device copy."""

    def __init__(self):
        self.buf = None
        self.qt = None
        self.event = None


_staging = _Staging()


def decode_coefficients(src):
    """Host half only: (JpegInfo, coefs int16 [coef_count] pinned CPU tensor view, qt int16-typed [192] CPU tensor holding
    uint16 values).  Exposed for the CPU tests; `imread` is the product entry."""
    data = _as_bytes(src)
    info = parse(data)
    st = _staging
    if st.event is not None:
        st.event.synchronize()
    if st.buf is None or st.buf.numel() < info.coef_count:
        pin = torch.cuda.is_available()
        st.buf = torch.empty(max(int(info.coef_count), 1 << 20), dtype=torch.int16, pin_memory=pin)
        st.qt = torch.empty(192, dtype=torch.int16, pin_memory=pin)
    L.check(L.lib().ymi_jpeg_decode_coefs(data, len(data), st.buf.data_ptr(), st.buf.numel(), st.qt.data_ptr(),
                                          C.byref(info.raw)), 'ymi_jpeg_decode_coefs')
    return info, st.buf[:info.coef_count], st.qt


def imread(src, device=None) -> torch.Tensor:
    """path | bytes -> uint8 BGR [h, w, 3] on `device` (default: the current CUDA device), EXIF orientation applied."""
    if not torch.cuda.is_available():
        raise RuntimeError('yolact_amd.data.jpeg.imread: no GPU — the pixel reconstruction runs on the device only '
                           '(the CPU oracle lives under oracle/ and is test-only)')
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    info, coefs, qt = decode_coefficients(src)
    with torch.cuda.device(device):
        coefs_d = coefs.to(device, non_blocking=True)
        qt_d = qt.to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _staging.event = ev
        planes = torch.empty(int(info.plane_bytes), dtype=torch.uint8, device=device)
        out = torch.empty((info.out_height, info.out_width, 3), dtype=torch.uint8, device=device)
        L.check(L.lib().ymi_jpeg_reconstruct_bgr_u8(C.byref(info.raw), coefs_d.data_ptr(), qt_d.data_ptr(), planes.data_ptr(),
                                                    out.data_ptr(), L.stream_ptr()), 'ymi_jpeg_reconstruct_bgr_u8')
    return out


_SUBSAMPLING = {'4:2:0': L.JPEG_SUB_420, '4:4:4': L.JPEG_SUB_444, '420': L.JPEG_SUB_420, '444': L.JPEG_SUB_444,
                L.JPEG_SUB_420: L.JPEG_SUB_420, L.JPEG_SUB_444: L.JPEG_SUB_444}


def _enc_args(h, w, quality, subsampling):
    if subsampling not in _SUBSAMPLING or isinstance(subsampling, bool):
        raise ValueError("subsampling: '4:2:0' or '4:4:4', got %r" % (subsampling,))
    if not isinstance(quality, int) or isinstance(quality, bool) or not 1 <= quality <= 100:
        raise ValueError('quality: an integer 1..100, got %r' % (quality,))
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError('JPEG holds 1..65535 pixels a side, got %d x %d' % (h, w))
    return _SUBSAMPLING[subsampling]


def write_header(h, w, quality=95, subsampling='4:2:0') -> bytes:
    """SOI .. SOS of the file `JpegEncoder` writes (host only)."""
    sub = _enc_args(h, w, quality, subsampling)
    buf = (C.c_uint8 * L.JPEG_HEADER_BYTES)()
    n = C.c_size_t()
    L.check(L.lib().ymi_jpeg_write_header(h, w, quality, sub, buf, len(buf), C.byref(n)), 'ymi_jpeg_write_header')
    return bytes(buf[:n.value])


class JpegEncoder:
    """Encoder for frames of one size: owns the device workspace, the device output buffer and the pinned read-back slots.

    A read-back copies the length and the first `guess` bytes of the stream in ONE device -> host transfer; `guess` starts at
    a quarter of the raw frame and follows the largest stream seen, so a second transfer (the rest of a stream that turned out
    longer) happens at most on the first frames of a harder sequence."""

    def __init__(self, h, w, quality=95, subsampling='4:2:0', device=None):
        if not torch.cuda.is_available():
            raise RuntimeError('yolact_amd.data.jpeg.JpegEncoder: no GPU — the encoder runs on the device only')
        self.h, self.w, self.quality = int(h), int(w), quality
        self.sub = _enc_args(self.h, self.w, quality, subsampling)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('yolact_amd.data.jpeg.JpegEncoder: device must be a GPU; there is no CPU encode path')
        self.header = write_header(self.h, self.w, quality, subsampling)
        d = L.JpegEncDesc(h=self.h, w=self.w, quality=quality, subsampling=self.sub)
        ws_bytes = L.lib().ymi_workspace_bytes(L.WS_JPEG_ENC, C.byref(d))
        self.cap = L.lib().ymi_workspace_bytes(L.WS_JPEG_ENC_OUT, C.byref(d))
        if ws_bytes < 0 or self.cap < 0:
            L.check(int(min(ws_bytes, self.cap)), 'ymi_workspace_bytes')
        self.ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=self.device)
        # [int64 length | stream]: one contiguous device range, so length + bytes leave in one copy
        self.out = torch.empty(8 + int(self.cap), dtype=torch.uint8, device=self.device)
        self.guess = min(int(self.cap), max(4096, self.h * self.w * 3 // 4))
        self._slots = []

    def _slot(self, i):
        while len(self._slots) <= i:
            self._slots.append(None)
        if self._slots[i] is None or self._slots[i].numel() < 8 + self.guess:
            self._slots[i] = torch.empty(8 + self.guess, dtype=torch.uint8, pin_memory=True)
        return self._slots[i]

    def _check(self, img):
        if not isinstance(img, torch.Tensor):
            raise TypeError('imencode: a uint8 BGR [h, w, 3] tensor on the GPU, got %r' % type(img))
        L.require_cuda(img, 'image')
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError('imencode: uint8 BGR [h, w, 3], got %s %s' % (img.dtype, tuple(img.shape)))
        if tuple(img.shape[:2]) != (self.h, self.w):
            raise ValueError('JpegEncoder built for %d x %d, got %d x %d' % (self.h, self.w, img.shape[0], img.shape[1]))
        if img.device != self.device:
            raise ValueError('JpegEncoder lives on %s, the image on %s' % (self.device, img.device))
        if img.stride(2) != 1 or img.stride(1) != 3 or img.stride(0) < 3 * self.w:
            img = img.contiguous()       # packed pixels and an arbitrary ROW stride go to the kernels as they are
        return img

    def _enqueue(self, img, slot):
        """Kernels + the read-back copy of frame `img` into pinned slot `slot`, all on the current stream."""
        img = self._check(img)
        d = L.JpegEncDesc(img=img.data_ptr(), h=self.h, w=self.w, row_stride=img.stride(0), quality=self.quality,
                          subsampling=self.sub, out=self.out.data_ptr() + 8, out_capacity=self.cap,
                          out_len=self.out.data_ptr(), ws=self.ws.data_ptr())
        L.check(L.lib().ymi_jpeg_encode_bgr_u8(C.byref(d), L.stream_ptr()), 'ymi_jpeg_encode_bgr_u8')
        n = 8 + self.guess
        self._slot(slot)[:n].copy_(self.out[:n], non_blocking=True)
        return img, self.guess

    def _finish(self, slot, img, copied):
        n = int(self._slots[slot][:8].view(torch.int64).item())
        if n > copied:
            # the stream outgrew the guess (self.out may hold a later frame by now): raise the guess, encode this frame again
            self.guess = min(int(self.cap), n + n // 4)
            self._enqueue(img, slot)
            torch.cuda.current_stream().synchronize()
        return self.header + self._slots[slot][8:8 + n].numpy().tobytes()

    def encode(self, img) -> bytes:
        """One frame -> the file bytes (header + scan + EOI)."""
        return self.encode_many([img])[0]

    def encode_many(self, frames) -> list:
        """Every frame is enqueued (kernels + its read-back) before the single synchronisation: the video case."""
        with torch.cuda.device(self.device):
            kept = [self._enqueue(f, i) for i, f in enumerate(frames)]
            torch.cuda.current_stream().synchronize()
            return [self._finish(i, img, copied) for i, (img, copied) in enumerate(kept)]


def imencode(img, quality=95, subsampling='4:2:0') -> bytes:
    """uint8 BGR [h, w, 3] on the GPU -> JPEG file bytes, what `cv2.imwrite` would put in the file (libjpeg defaults: baseline,
    4:2:0, quality 95)."""
    if not isinstance(img, torch.Tensor):
        raise TypeError('imencode: a uint8 BGR [h, w, 3] tensor on the GPU, got %r' % type(img))
    L.require_cuda(img, 'image')
    if img.dim() != 3:
        raise ValueError('imencode: uint8 BGR [h, w, 3], got %s' % (tuple(img.shape),))
    return JpegEncoder(img.shape[0], img.shape[1], quality, subsampling, img.device).encode(img)


def imwrite(path, img, quality=95, subsampling='4:2:0') -> bool:
    """`cv2.imwrite(path, img)` for a .jpg path and a frame on the GPU (eval.py evalimage: `cv2.imwrite(save_path, img_numpy)`)."""
    data = imencode(img, quality, subsampling)
    with open(path, 'wb') as f:
        f.write(data)
    return True
