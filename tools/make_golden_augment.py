"""Generate tests/golden/augment_draws.npz by EXECUTING THE REFERENCE's own SSDAugmentation object (build container only; no test
runs this).

    python tools/make_golden_augment.py            # needs the reference checkout; writes tests/golden/augment_draws.npz

Every random decision of the reference's training transform depends on the image size, the boxes, the labels and num_crowds only,
never on a pixel value.  So the reference's utils.augmentations is imported with the stubs of oracle/make_golden._shim_reference and a
`cv2` stub whose cvtColor returns its input and whose resize returns an array of the requested size (cv2 is not installed): the
transform then makes exactly the draws it makes in training, on images of zeros.  The installed numpy refuses random.choice on the
ragged `sample_options` tuple, so that INSTANCE ATTRIBUTE is set to a 1-D object array of the same six entries (data, not code).

Per run (a case under numpy.random.seed(seed)) the file holds the output boxes, labels and num_crowds, the shape of the image that
reached Resize, and one further numpy.random.uniform() drawn after the call: equal only if the same number of draws was consumed.
The cases' inputs are stored too, so the test needs nothing else.  Coverage is checked here and the tool fails without it: every crop
option, a crop that exhausts its 50 trials, an expansion, a mirror, a case with crowds, a run where Resize's discard drops a box.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

SEEDS = range(24)
MAX_BYTES = 64 * 1024

# name, height, width, relative boxes, labels (crowds last, -1), num_crowds
CASES = [
    ('coco', 480, 640, [[0.10, 0.20, 0.45, 0.70], [0.30, 0.25, 0.90, 0.95], [0.55, 0.05, 0.75, 0.40], [0.02, 0.60, 0.20, 0.98],
                        [0.40, 0.45, 0.60, 0.62], [0.70, 0.55, 0.98, 0.80], [0.15, 0.05, 0.35, 0.18]],
     [0, 17, 17, 56, 2, 61, 79], 0),
    ('crowds', 375, 500, [[0.05, 0.10, 0.50, 0.60], [0.45, 0.35, 0.95, 0.90], [0.20, 0.55, 0.40, 0.85], [0.00, 0.00, 1.00, 0.50],
                          [0.60, 0.05, 0.95, 0.35]],
     [14, 0, 39, -1, -1], 2),
    ('corner', 100, 160, [[0.000, 0.000, 0.020, 0.030]], [5], 0),                   # a crop rarely holds this centre: 50 trials run out
    ('sliver', 53, 37, [[0.30, 0.20, 0.30, 0.60], [0.10, 0.10, 0.80, 0.85], [0.50, 0.40, 0.95, 0.90]], [1, 2, 3], 0),   # zero width
    ('tall', 640, 427, [[0.25, 0.05, 0.75, 0.50], [0.10, 0.50, 0.60, 0.99], [0.55, 0.60, 0.58, 0.61], [0.0, 0.0, 1.0, 1.0]],
     [0, 0, 24, -1], 1),
]


def main():
    from make_golden import _shim_reference
    _shim_reference()
    import cv2
    log = {}

    def resize(img, size):
        log.setdefault('resized', []).append(img)
        width, height = size
        out = np.zeros((height, width) + tuple(img.shape[2:]), dtype=img.dtype)
        return out[:, :, 0] if (out.ndim == 3 and out.shape[2] == 1) else out

    cv2.cvtColor = lambda img, code: img
    cv2.resize = resize
    cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = 40, 54
    from data import MEANS, set_cfg
    import utils.augmentations as A
    set_cfg('yolact_base_config')

    real_choice, real_uniform = np.random.choice, np.random.uniform

    def choice(a, *args, **kw):
        got = real_choice(a, *args, **kw)
        log.setdefault('modes', []).append(got)
        return got

    def uniform(*args, **kw):
        log.setdefault('uniform', []).append(args)
        return real_uniform(*args, **kw)

    aug = A.SSDAugmentation(MEANS)
    crop = [t for t in aug.augment.transforms if isinstance(t, A.RandomSampleCrop)][0]
    options = np.empty(len(crop.sample_options), dtype=object)
    for i, o in enumerate(crop.sample_options):
        options[i] = o
    crop.sample_options = options

    out = {'case_name': np.array([c[0] for c in CASES]), 'case_hw': np.array([c[1:3] for c in CASES]),
           'case_boxes': np.concatenate([np.array(c[3], dtype=np.float64) for c in CASES]),
           'case_labels': np.concatenate([np.array(c[4], dtype=np.float64) for c in CASES]),
           'case_off': np.cumsum([0] + [len(c[3]) for c in CASES]), 'case_num_crowds': np.array([c[5] for c in CASES])}
    runs = {k: [] for k in ('case', 'seed', 'boxes', 'labels', 'num_crowds', 'pre_shape', 'trail')}
    seen = {'modes': set(), 'exhausted': 0, 'expand': 0, 'mirror': 0, 'crowds': 0, 'discard': 0}
    for ci, (name, h, w, boxes, labels, num_crowds) in enumerate(CASES):
        for seed in SEEDS:
            log.clear()
            A.random.choice, A.random.uniform = choice, uniform          # numpy.random itself: restored below
            try:
                np.random.seed(seed)
                img = np.zeros((h, w, 3), dtype=np.uint8)
                masks = np.zeros((len(boxes), h, w), dtype=np.uint8)
                _, m_out, b_out, l_out = aug(img, masks, np.array(boxes, dtype=np.float64),
                                             {'num_crowds': num_crowds, 'labels': np.array(labels, dtype=np.float64)})
            finally:
                A.random.choice, A.random.uniform = real_choice, real_uniform
            trail = np.random.uniform()
            pre, pre_masks = log['resized'][0], log['resized'][1]
            assert m_out.shape[0] == b_out.shape[0] == l_out['labels'].shape[0]
            runs['case'].append(ci)
            runs['seed'].append(seed)
            runs['boxes'].append(np.array(b_out, dtype=np.float64).reshape(-1, 4))
            runs['labels'].append(np.array(l_out['labels'], dtype=np.float64))
            runs['num_crowds'].append(int(l_out['num_crowds']))
            runs['pre_shape'].append(pre.shape[:2])
            runs['trail'].append(trail)
            modes = log['modes']
            seen['modes'] |= {options.tolist().index(m) for m in modes}
            seen['exhausted'] += len(modes) > 1 and any(m is not None for m in modes[:-1])
            seen['expand'] += any(a == (1, 4) for a in log['uniform'])
            seen['mirror'] += pre.strides[1] < 0
            seen['crowds'] += int(l_out['num_crowds']) > 0
            seen['discard'] += b_out.shape[0] < pre_masks.shape[2]
    print('coverage:', seen)
    assert seen['modes'] == set(range(6)), 'a crop option was never chosen'
    for k in ('exhausted', 'expand', 'mirror', 'crowds', 'discard'):
        assert seen[k] > 0, 'no run with: ' + k
    out.update(run_case=np.array(runs['case']), run_seed=np.array(runs['seed']), run_boxes=np.concatenate(runs['boxes']),
               run_labels=np.concatenate(runs['labels']), run_off=np.cumsum([0] + [len(b) for b in runs['boxes']]),
               run_num_crowds=np.array(runs['num_crowds']), run_pre_shape=np.array(runs['pre_shape']),
               run_trail=np.array(runs['trail']))
    path = os.path.join(ROOT, 'tests', 'golden', 'augment_draws.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('%d runs over %d cases -> %s (%d bytes)' % (len(runs['case']), len(CASES), path, size))
    assert len(runs['case']) >= 64 and len(CASES) >= 4 and size <= MAX_BYTES


if __name__ == '__main__':
    main()
