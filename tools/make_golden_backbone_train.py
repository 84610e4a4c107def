"""Generate tests/golden/backbone_train.npz by EXECUTING THE REFERENCE's own backbone.Bottleneck class on the CPU (build container only).

    python tools/make_golden_backbone_train.py            # needs the reference checkout; writes tests/golden/backbone_train.npz
    python tools/make_golden_backbone_train.py --search N # which of the seeds 1 .. N qualify (needs no reference)

The reference is imported with the stubs of oracle/make_golden._shim_reference.  The model is
Bottleneck(64, 32, stride=2, downsample=Sequential(Conv2d(64, 128, 1, stride=2, bias=False), BatchNorm2d(128))) followed by
Bottleneck(128, 32), on an input of [2, 64, 9, 7], which gives [2, 128, 5, 4]: a stride-2 3x3 and a stride-2 projection on odd
extents, then an identity block.  It runs once with the BatchNorm modules in eval mode (the running statistics as they are) and once in
train mode (batch statistics, the running ones updated).  Stored:

    x, p_<name>, up          the input, every parameter and running statistic before the step, and the upstream gradient G of the
                             output (values in {-1, -1/2, 0, 1/2, 1}), all on fp16-exact grids, as fp16
                             (tests/backbone_train_ref.random_case, seed SEED)
    eval_y, train_y          the reference's outputs
    <mode>_d_x, <mode>_d_<name>   the gradients of <y, G> in x, in every convolution weight and in every BatchNorm weight and bias
    train_new_<name>         the running statistics after the train-mode step

as fp32.  A seed of 1 .. 64 qualifies when every ReLU input that receives gradient keeps 16 times that tensor's fp32-versus-fp64
deviation as margin in BOTH modes; the seed used is the qualifying one with the WIDEST margin (the fp32 deviation differs a little from
host to host), and it and the number that qualify are written into the meta.  Only data is stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEARCHED = 64


def qualifies(R, seed):
    x, params, blocks, up = R.random_case(seed, R.GOLDEN_X, R.GOLDEN_BLOCKS)
    t = [R.tightest(R.relu_margins(x, params, blocks, up, mode)) for mode in (False, True)]
    return all(lo >= 16 * dev for _, lo, dev in t), t


def search(R, n, verbose=True):
    """-> the qualifying seeds, the one with the widest margin (the smaller of its two modes' margin / deviation) first."""
    good, width = [], {}
    for seed in range(1, n + 1):
        ok, t = qualifies(R, seed)
        if ok:
            good.append(seed)
            width[seed] = min(lo / max(dev, 1e-300) for _, lo, dev in t)
        if verbose:
            print('seed %3d: %s  eval %s %.3e / %.3e   train %s %.3e / %.3e' % ((seed, ok) + t[0] + t[1]))
    good.sort(key=lambda sd: -width[sd])
    print('%d of the seeds 1 .. %d qualify, widest margin first: %s' % (len(good), n, good))
    if good:
        print('seed %d keeps %.1f times the deviation' % (good[0], width[good[0]]))
    return good


def main():
    import backbone_train_ref as R
    if len(sys.argv) > 2 and sys.argv[1] == '--search':
        return search(R, int(sys.argv[2]))
    good = search(R, SEARCHED, verbose=False)
    seed = good[0]
    from oracle.make_golden import _shim_reference
    _shim_reference()
    import backbone as ref_backbone
    (i0, p0, s0, _), (i1, p1, s1, _) = R.GOLDEN_BLOCKS
    model = nn.Sequential(
        ref_backbone.Bottleneck(i0, p0, stride=s0, downsample=nn.Sequential(nn.Conv2d(i0, 4 * p0, 1, stride=s0, bias=False),
                                                                           nn.BatchNorm2d(4 * p0))),
        ref_backbone.Bottleneck(i1, p1))
    x, params, blocks, up = R.random_case(seed, R.GOLDEN_X, R.GOLDEN_BLOCKS)
    sd = model.state_dict()
    names = list(params)
    assert sorted(names) == sorted(k for k in sd if 'num_batches' not in k), (names, list(sd))
    torch.set_num_threads(R.helpers.ORACLE_THREADS)     # the thread count the oracle runs with on every host

    arrays = {'x': x.numpy().astype(np.float16), 'up': up.numpy().astype(np.float16)}
    for n in names:
        arrays['p_' + n] = params[n].numpy().astype(np.float16)
        assert np.array_equal(arrays['p_' + n].astype(np.float32), params[n].numpy())
    results = {}
    for mode, train in (('eval', False), ('train', True)):
        with torch.no_grad():
            for n in names:
                assert sd[n].shape == params[n].shape, n
                sd[n].copy_(params[n])
        model.train(train)
        leaf = x.clone().requires_grad_(True)
        y = model(leaf)
        assert tuple(y.shape) == (2, 128, 5, 4)
        named = dict(model.named_parameters())
        leaves = [n for n in names if R.is_leaf_name(n)]
        grads = torch.autograd.grad((y * up).sum(), [leaf] + [named[n] for n in leaves])
        res = {'y': y.detach(), 'd_x': grads[0]}
        res.update({'d_' + n: g for n, g in zip(leaves, grads[1:])})
        if train:
            res.update({'new_' + n: sd[n].detach().clone() for n in names if not R.is_leaf_name(n)})
        for k, v in res.items():
            arrays['%s_%s' % (mode, k)] = v.numpy().astype(np.float32)
        results[mode] = res
        # the plain-torch restatement agrees with what the reference just computed
        for dtype in (torch.float32, torch.float64):
            r = R.run_ref(x, params, blocks, up, train, dtype)
            worst = max(R.rel_err(r[k], res[k]) for k in res)
            print('%s, oracle %s: largest rel_err against the reference %.3e' % (mode, dtype, worst))
            assert worst <= 1e-6

    margins = {mode: R.tightest(R.relu_margins(x, params, blocks, up, train)) for mode, train in (('eval', False), ('train', True))}
    meta = dict(seed=seed, searched=SEARCHED, qualified=len(good), x=list(R.GOLDEN_X), blocks=[[p, s] for p, s in blocks],
                specs=[list(s) for s in R.GOLDEN_BLOCKS], params=names, eps=R.EPS, momentum=R.MOMENTUM,
                tightest_margin={m: [t[0], t[1], t[2]] for m, t in margins.items()}, torch=torch.__version__)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'backbone_train.npz')
    np.savez_compressed(out, **arrays)
    print('seed', seed, 'of', len(good), 'qualified; wrote', out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg.npz'))      # the largest fixture


if __name__ == '__main__':
    main()
