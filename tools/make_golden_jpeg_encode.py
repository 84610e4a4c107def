#!/usr/bin/env python
"""Writes tests/golden/jpeg_encode.npz: for every case of tests/jpeg_enc_cases.py the input pixels and the bytes Pillow
(libjpeg-turbo) writes for them — `Image.fromarray(rgb).save(buf, 'JPEG', quality=q, subsampling=2 or 0)`, the library's
defaults otherwise (baseline, standard Huffman tables, ISLOW DCT).  The two photo-sized cases are stored as the SHA-256 and
the length of Pillow's bytes only.  Needs Pillow; nothing of this project's encoder runs here."""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpeg_enc_cases as K      # noqa: E402


def pillow_bytes(bgr, quality, sub):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, 'JPEG', quality=quality, subsampling=sub)
    return buf.getvalue()


def main():
    import PIL
    from PIL import features
    out = {'versions': np.array(['Pillow ' + PIL.__version__, 'libjpeg-turbo ' + str(features.version_feature('libjpeg_turbo'))])}
    for name, content, h, w, q, s in K.cases():
        px = K.pixels(content, h, w)
        out.setdefault('px_%dx%d_%s' % (h, w, content), px)
        out['jpg_' + name] = np.frombuffer(pillow_bytes(px, q, K.SUBS[s]), dtype=np.uint8)
    for h, w, seed in K.LARGE:
        data = pillow_bytes(K.frame(h, w, seed), 95, 2)
        out['big_%dx%d_sha256' % (h, w)] = np.frombuffer(hashlib.sha256(data).digest(), dtype=np.uint8)
        out['big_%dx%d_len' % (h, w)] = np.array(len(data), dtype=np.int64)
    path = os.path.join(ROOT, 'tests', 'golden', 'jpeg_encode.npz')
    np.savez_compressed(path, **out)
    print('%s: %d cases, %d bytes' % (path, len(K.cases()), os.path.getsize(path)))


if __name__ == '__main__':
    main()
