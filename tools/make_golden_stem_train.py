"""Generate tests/golden/stem_train.npz by EXECUTING THE REFERENCE's own backbone.ResNetBackbone object's stem on the CPU (build
container only).

    python tools/make_golden_stem_train.py            # needs the reference checkout; writes tests/golden/stem_train.npz
    python tools/make_golden_stem_train.py --search N # which of the seeds 1 .. N qualify (needs no reference)

The reference is imported with the stubs of oracle/make_golden._shim_reference.  The object is ResNetBackbone([3, 4, 6, 3]); its conv1,
bn1, relu and maxpool are called in its forward's order (backbone.py:129-132) on an input of [2, 3, 29, 23], which the convolution
takes to 15 x 12 and the pool to 8 x 6: odd and even extents in both.  It runs once with bn1 in eval mode (the running statistics as they
are) and once in train mode (batch statistics, the running ones updated).  Stored:

    x, p_<name>, up          the image, conv1.weight, bn1's parameters and running statistics before the step, and the upstream
                             gradient G of the pooled map (values in {-1, -1/2, 0, 1/2, 1}), all on fp16-exact grids, as fp16
                             (tests/stem_train_ref.random_case, seed SEED)
    eval_y, train_y          the reference's outputs
    <mode>_d_<name>          the gradients of <y, G> in conv1.weight, bn1.weight and bn1.bias
    train_new_<name>         the running statistics after the train-mode step

as fp32.  A seed of 1 .. 64 qualifies when, in BOTH modes, every ReLU input that receives gradient keeps 16 times that tensor's
fp32-versus-fp64 deviation from 0 and every pool window that receives gradient keeps 16 times the deviation of the pool's input between
its maximum and its largest smaller value (tests/stem_train_ref.margins); the seed used is the qualifying one with the WIDEST margin,
and it, the number that qualify and the margins are written into the meta.  Only data is stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEARCHED = 64
MAX_BYTES = 652222
MODES = (('eval', False), ('train', True))


def qualifies(R, seed):
    x, params, up = R.random_case(seed)
    m = [t for _, train in MODES for t in R.margins(x, params, up, train)]
    return all(lo >= 16 * dev for _, lo, dev in m), m


def search(R, n, verbose=True):
    """-> the qualifying seeds, the one with the widest margin (the smallest margin / deviation of its two modes) first."""
    good, width = [], {}
    for seed in range(1, n + 1):
        ok, m = qualifies(R, seed)
        if ok:
            good.append(seed)
            width[seed] = min(lo / max(dev, 1e-300) for _, lo, dev in m)
        if verbose:
            print('seed %3d: %s  %s' % (seed, ok, '  '.join('%s %.3e / %.3e' % t for t in m)))
    good.sort(key=lambda sd: -width[sd])
    print('%d of the seeds 1 .. %d qualify, widest margin first: %s' % (len(good), n, good))
    if good:
        print('seed %d keeps %.1f times the deviation' % (good[0], width[good[0]]))
    return good


def main():
    import stem_train_ref as R
    if len(sys.argv) > 2 and sys.argv[1] == '--search':
        return search(R, int(sys.argv[2]))
    good = search(R, SEARCHED, verbose=False)
    seed = good[0]
    from oracle.make_golden import _shim_reference
    _shim_reference()
    import backbone as ref_backbone
    bb = ref_backbone.ResNetBackbone([3, 4, 6, 3])
    x, params, up = R.random_case(seed)
    names = list(R.PARAM_NAMES)
    sd = {n: t for n, t in bb.state_dict().items() if n in names}
    assert sorted(sd) == sorted(names), list(sd)
    torch.set_num_threads(R.helpers.ORACLE_THREADS)     # the thread count the oracle runs with on every host

    arrays = {'x': x.numpy().astype(np.float16), 'up': up.numpy().astype(np.float16)}
    for n in names:
        arrays['p_' + n] = params[n].numpy().astype(np.float16)
        assert np.array_equal(arrays['p_' + n].astype(np.float32), params[n].numpy())
    for mode, train in MODES:
        with torch.no_grad():
            for n in names:
                assert sd[n].shape == params[n].shape, n
                sd[n].copy_(params[n])
        bb.train(train)
        y = bb.maxpool(bb.relu(bb.bn1(bb.conv1(x.clone()))))          # backbone.py:129-132
        assert tuple(y.shape) == (2, 64, 8, 6)
        named = dict(bb.named_parameters())
        grads = torch.autograd.grad((y * up).sum(), [named[n] for n in R.LEAVES])
        res = {'y': y.detach()}
        res.update({'d_' + n: g for n, g in zip(R.LEAVES, grads)})
        if train:
            res.update({'new_' + n: sd[n].detach().clone() for n in R.STATS})
        for k, v in res.items():
            arrays['%s_%s' % (mode, k)] = v.numpy().astype(np.float32)
        # the plain-torch restatement agrees with what the reference just computed
        for dtype in (torch.float32, torch.float64):
            r = R.run_ref(x, params, up, train, dtype)
            worst = max(R.rel_err(r[k], res[k]) for k in res)
            print('%s, oracle %s: largest rel_err against the reference %.3e' % (mode, dtype, worst))
            assert worst <= 1e-6

    margins = {mode: R.margins(x, params, up, train) for mode, train in MODES}
    meta = dict(seed=seed, searched=SEARCHED, qualified=len(good), x=list(R.GOLDEN_X), cout=R.GOLDEN_COUT, params=names, eps=R.EPS,
                momentum=R.MOMENTUM, margins={m: [list(t) for t in v] for m, v in margins.items()}, torch=torch.__version__)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'stem_train.npz')
    np.savez_compressed(out, **arrays)
    print('seed', seed, 'of', len(good), 'qualified; wrote', out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) <= MAX_BYTES


if __name__ == '__main__':
    main()
