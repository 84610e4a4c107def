"""Inputs of the JPEG encoder tests, shared by tools/make_golden_jpeg_encode.py (which asks Pillow / libjpeg-turbo for the
expected bytes) and the tests that read tests/golden/jpeg_encode.npz.  Integer arithmetic only, so the pixels do not depend
on a random generator's version.  Images are uint8 BGR [h, w, 3], what display.prep_display and data.jpeg.imread produce."""
import numpy as np

SIZES = [(1, 1), (7, 9), (8, 8), (15, 16), (16, 16), (17, 33), (37, 53), (64, 48), (100, 75)]      # (h, w)
CONTENTS = ['noise', 'grad', 'zero', 'white', 'checker', 'frame']
QUALITIES = [1, 50, 75, 95, 100]
SUBS = {'420': 2, '444': 0}                 # name -> Pillow's `subsampling` = YMI_JPEG_SUB_*
# every quality x both subsamplings on these; quality 95 / 4:2:0 on everything
SWEEP_SIZES = [(16, 16), (17, 33), (37, 53)]
SWEEP_CONTENTS = ['noise', 'checker', 'frame']
LARGE = [(480, 640, 11), (550, 550, 12)]    # (h, w, seed): stored as SHA-256 + length only


def _hash(h, w, seed):
    """[h, w, 3] uint32 of well-mixed bits (an integer hash of the coordinates)."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(3, dtype=np.uint64),
                          indexing='ij')
    v = (x * np.uint64(73856093)) ^ (y * np.uint64(19349663)) ^ (c * np.uint64(83492791)) ^ np.uint64(seed * 2654435761 + 97)
    for _ in range(2):
        v = (v ^ (v >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
        v = (v ^ (v >> np.uint64(13))) * np.uint64(3266489917) & np.uint64(0xFFFFFFFF)
    return (v ^ (v >> np.uint64(16))).astype(np.uint32)


def frame(h, w, seed):
    """A composited-looking frame: a smooth background, flat mask-coloured rectangles blended over it, mild sensor noise."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    img = np.stack([(x * 200) // max(w, 1) + 20, (y * 180) // max(h, 1) + 40, ((x + 2 * y) * 150) // max(w + 2 * h, 1) + 60], -1)
    img = img + (_hash(h, w, seed).astype(np.int64) % 7) - 3
    for k in range(5):
        hs = _hash(1, 8, seed * 31 + k).reshape(-1).astype(np.int64)
        y0, x0 = hs[0] % max(h, 1), hs[1] % max(w, 1)
        y1, x1 = min(h, y0 + 1 + hs[2] % max(h // 2, 1)), min(w, x0 + 1 + hs[3] % max(w // 2, 1))
        colour = np.array([hs[4] % 256, hs[5] % 256, hs[6] % 256])
        img[y0:y1, x0:x1] = (img[y0:y1, x0:x1] * 140 + colour * 116) // 256        # alpha 0.45 like the mask overlay
    return np.clip(img, 0, 255).astype(np.uint8)


def pixels(content, h, w, seed=0):
    if content == 'noise':
        return (_hash(h, w, seed + 1000 * h + w) & 255).astype(np.uint8)
    if content == 'grad':
        y, x = np.mgrid[0:h, 0:w].astype(np.int64)
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)],
                        -1).astype(np.uint8)
    if content == 'zero':
        return np.zeros((h, w, 3), np.uint8)
    if content == 'white':
        return np.full((h, w, 3), 255, np.uint8)
    if content == 'checker':
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    if content == 'frame':
        return frame(h, w, seed + h * 7 + w)
    raise KeyError(content)


def cases():
    """[(name, content, h, w, quality, sub name)] in a fixed order."""
    out = []
    for h, w in SIZES:
        for c in CONTENTS:
            out.append(('%dx%d_%s_q95_420' % (h, w, c), c, h, w, 95, '420'))
    for h, w in SWEEP_SIZES:
        for c in SWEEP_CONTENTS:
            for q in QUALITIES:
                for s in SUBS:
                    if (q, s) != (95, '420'):
                        out.append(('%dx%d_%s_q%d_%s' % (h, w, c, q, s), c, h, w, q, s))
    return out
