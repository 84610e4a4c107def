"""Child process of tests/test_gpu_mask_kat.py::test_env_variants_write_the_same_bits: the upsample's A/B switches are read once per
process (a static in csrc/mask.hip), so each setting needs a process of its own.  Runs the first two shapes of UP_CASES on the
three inputs under whatever YOLACT_AMD_UPSAMPLE / YOLACT_AMD_UPSAMPLE_FLAT the parent set, and saves the soft outputs (fp32), the
hard ones (uint8 after checking that they are exactly 0 / 1) and the kernel the library says it ran.  Usage: mask_kat_child.py OUTDIR"""
import json
import os
import sys
import time

T0 = time.time()
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main(outdir):
    import numpy as np
    import torch
    import test_gpu_mask_kat as K
    meta = {}
    t1 = time.time()
    for ci in (0, 1):
        name, ph, pw, h, w, nmask, _ = K.UP_CASES[ci]
        for kind in K.MR.UP_INPUTS:
            lo = torch.from_numpy(K.case_input(ci, kind)).to(K.DEV)
            soft, k_soft = K.run_upsample(lo, nmask, ph, pw, h, w, -1.0)
            hard, k_hard = K.run_upsample(lo, nmask, ph, pw, h, w, 0.5)
            assert k_soft == k_hard and bool(((hard == 0) | (hard == 1)).all())
            np.save(os.path.join(outdir, 'soft_%d_%s.npy' % (ci, kind)), soft)
            np.save(os.path.join(outdir, 'hard_%d_%s.npy' % (ci, kind)), hard.astype(np.uint8))
            meta['%d_%s' % (ci, kind)] = k_soft
    meta['seconds_work'], meta['seconds_total'] = time.time() - t1, time.time() - T0
    with open(os.path.join(outdir, 'meta.json'), 'w') as f:
        json.dump(meta, f)


if __name__ == '__main__':
    main(sys.argv[1])
