#!/usr/bin/env python
"""Throughput of the pull_item image read: host entropy decode, H2D copy + device reconstruction, and the whole
pull_item-style chain (imread -> BaseTransform) on a photo-sized 4:2:0 file (641x427, restart interval 7).

--encode: the write side (data.jpeg.JpegEncoder) at 480x640 and 550x550, quality 95, 4:2:0, 64 different frames: device time
per frame from events around the 64 enqueued encodes, wall time per frame of encode_many including the read-back, and Pillow
(libjpeg-turbo) encoding the same frames on this machine's host CPU in the same process."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def photo_sized_jpeg():
    """641x427 4:2:0 baseline file with restart markers, written by Pillow (no oracle / test code in a measurement tool)."""
    import io
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(8)
    h, w = 427, 641
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(xx / 17.0 + yy / 23.0), 128 + 90 * np.cos(xx / 11.0) * np.sin(yy / 19.0),
                    (xx + yy) * 255.0 / (w + h)], -1) + rng.normal(0, 10, (h, w, 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, 'JPEG', quality=85, subsampling=2, restart_marker_blocks=7)
    return buf.getvalue()


def synthetic_frames(h, w, n):
    """n different composited-looking uint8 BGR frames (smooth background, flat blended rectangles, mild noise)."""
    import numpy as np
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        img = np.stack([128 + 100 * np.sin(xx / 37.0 + yy / 53.0 + i), 128 + 90 * np.cos(xx / 41.0) * np.sin(yy / 29.0 + i),
                        (xx + yy) * 255.0 / (w + h)], -1) + rng.normal(0, 3, (h, w, 3))
        for _ in range(5):
            y0, x0 = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
            y1, x1 = y0 + int(rng.integers(40, h // 2)), x0 + int(rng.integers(40, w // 2))
            img[y0:y1, x0:x1] = img[y0:y1, x0:x1] * 0.55 + rng.integers(0, 256, 3) * 0.45
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def encode_mode():
    import io
    import PIL
    from PIL import Image, features
    from yolact_amd.data import jpeg
    res = {'mode': 'encode', 'quality': 95, 'subsampling': '4:2:0', 'frames': 64,
           'pillow': PIL.__version__, 'libjpeg_turbo': str(features.version_feature('libjpeg_turbo'))}
    for h, w in ((480, 640), (550, 550)):
        host = synthetic_frames(h, w, 64)
        dev = [torch.from_numpy(f).cuda() for f in host]
        enc = jpeg.JpegEncoder(h, w, 95, '4:2:0')
        for _ in range(3):
            files = enc.encode_many(dev)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dev_ms, wall_ms = [], []
        for _ in range(5):
            e0.record()
            for i, f in enumerate(dev):
                enc._enqueue(f, i)
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1) / len(dev))
            t0 = time.perf_counter()
            files = enc.encode_many(dev)
            wall_ms.append((time.perf_counter() - t0) / len(dev) * 1e3)
        pil_ms, same = [], True
        for _ in range(3):
            t0 = time.perf_counter()
            ref = []
            for f in host:
                buf = io.BytesIO()
                Image.fromarray(f[..., ::-1]).save(buf, 'JPEG', quality=95, subsampling=2)
                ref.append(buf.getvalue())
            pil_ms.append((time.perf_counter() - t0) / len(host) * 1e3)
        same = ref == files
        key = '%dx%d' % (h, w)
        res[key] = {'device_ms_per_frame': round(min(dev_ms), 4), 'device_ms_per_frame_median': round(sorted(dev_ms)[2], 4),
                    'wall_ms_per_frame': round(min(wall_ms), 4), 'wall_ms_per_frame_median': round(sorted(wall_ms)[2], 4),
                    'pillow_host_ms_per_frame': round(min(pil_ms), 4), 'bytes_equal_pillow': bool(same),
                    'mean_file_bytes': int(sum(len(x) for x in files) / len(files)), 'raw_bytes': h * w * 3}
    print(json.dumps(res))


def main():
    if '--encode' in sys.argv[1:]:
        return encode_mode()
    import yolact_amd
    from yolact_amd.data import jpeg
    from yolact_amd.utils.augmentations import BaseTransform
    yolact_amd.set_cfg('yolact_resnet50_config')
    data = photo_sized_jpeg()
    res = {'file_bytes': len(data), 'image': '641x427 4:2:0'}
    n = 200
    t0 = time.perf_counter()
    for _ in range(n):
        jpeg.decode_coefficients(data)
    res['host_entropy_decode_ms'] = round((time.perf_counter() - t0) / n * 1e3, 3)
    tr = BaseTransform()
    for fn, key in ((lambda: jpeg.imread(data), 'imread_ms'), (lambda: tr(jpeg.imread(data))[0], 'imread_plus_base_transform_ms')):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        res[key] = round((time.perf_counter() - t0) / n * 1e3, 3)
    res['images_per_s_one_host_thread'] = round(1e3 / res['imread_plus_base_transform_ms'], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
