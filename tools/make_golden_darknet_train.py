"""Generate tests/golden/darknet_train.npz by EXECUTING THE REFERENCE's own backbone.darknetconvlayer and backbone.DarkNetBlock on the CPU
in fp64 (build container only).

    python tools/make_golden_darknet_train.py            # needs the reference checkout; writes tests/golden/darknet_train.npz
    python tools/make_golden_darknet_train.py --search N # which of the seeds 1 .. N qualify (needs no reference)

The reference is imported with the stubs of oracle/make_golden._shim_reference.  Three cases (tests/darknet_train_ref.GOLDEN_CASES):

    pre     darknetconvlayer(3, 32, 3, padding=1) on [2, 3, 9, 7]: the pre-convolution
    down    darknetconvlayer(32, 64, 3, stride=2, padding=1) on [2, 32, 9, 7] -> [2, 64, 5, 4]: a stage's first unit on odd extents
    block   DarkNetBlock(64, 32) on [2, 64, 9, 7]: the residual behind the activation

Each runs once with its BatchNorm modules in eval mode (the running statistics as they are) and once in train mode (batch statistics,
the running ones updated), the whole module converted to fp64.  Stored per case, under '<case>_':

    x, p_<name>, up          the input, every parameter and running statistic before the step, and the upstream gradient G of the
                             output (values in {-1, -1/2, 0, 1/2, 1}), all on fp16-exact grids, as fp16
                             (tests/darknet_train_ref.random_case, the case's seed)
    eval_y, train_y          the reference's outputs
    <mode>_d_x, <mode>_d_<name>   the gradients of <y, G> in x, in every convolution weight and in every BatchNorm weight and bias
    train_new_<name>         the running statistics after the train-mode step

as fp32.  A seed of 1 .. 64 qualifies when every LeakyReLU input that receives gradient keeps 16 times that tensor's fp32-versus-fp64
deviation as margin in BOTH modes; the seed used is the qualifying one with the WIDEST margin, and it and the number that qualify are
written into the meta.  Only data is stored.
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
MODES = (('eval', False), ('train', True))


def search(R, case, n, verbose=True):
    """-> the qualifying seeds of a case, the one with the widest margin (the smaller of its two modes' margin / deviation) first."""
    net, xshape, shapes = R.GOLDEN_CASES[case]
    good, width = [], {}
    for seed in range(1, n + 1):
        x, params, ups = R.random_case(seed, xshape, net, shapes)
        t = [R.tightest(R.leaky_margins(x, params, net, ups, train)) for _, train in MODES]
        ok = all(lo >= 16 * dev for _, lo, dev in t)
        if ok:
            good.append(seed)
            width[seed] = min(lo / max(dev, 1e-300) for _, lo, dev in t)
        if verbose:
            print('%s seed %3d: %s  eval %s %.3e / %.3e   train %s %.3e / %.3e' % ((case, seed, ok) + t[0] + t[1]))
    good.sort(key=lambda sd: -width[sd])
    print('%s: %d of the seeds 1 .. %d qualify, widest margin first: %s' % (case, len(good), n, good))
    return good


def build(ref_backbone, case):
    if case == 'pre':
        return ref_backbone.darknetconvlayer(3, 32, 3, padding=1)
    if case == 'down':
        return ref_backbone.darknetconvlayer(32, 64, 3, stride=2, padding=1)
    return ref_backbone.DarkNetBlock(64, 32)


def main():
    import darknet_train_ref as R
    if len(sys.argv) > 2 and sys.argv[1] == '--search':
        return [search(R, case, int(sys.argv[2])) for case in R.GOLDEN_CASES]
    from oracle.make_golden import _shim_reference
    _shim_reference()
    import backbone as ref_backbone
    torch.set_num_threads(R.helpers.ORACLE_THREADS)     # the thread count the oracle runs with on every host
    arrays, meta = {}, dict(cases=list(R.GOLDEN_CASES), searched=SEARCHED, seed={}, qualified={}, params={}, x={}, tightest_margin={},
                            eps=R.EPS, momentum=R.MOMENTUM, slope=R.SLOPE, torch=torch.__version__)
    for case, (net, xshape, shapes) in R.GOLDEN_CASES.items():
        good = search(R, case, SEARCHED, verbose=False)
        seed = good[0]
        x, params, ups = R.random_case(seed, xshape, net, shapes)
        up = ups[0]
        model = build(ref_backbone, case).double()
        sd = model.state_dict()
        names = list(params)
        assert sorted(names) == sorted(k for k in sd if 'num_batches' not in k), (names, list(sd))
        pre = case + '_'
        arrays[pre + 'x'], arrays[pre + 'up'] = x.numpy().astype(np.float16), up.numpy().astype(np.float16)
        for n in names:
            arrays[pre + 'p_' + n] = params[n].numpy().astype(np.float16)
            assert np.array_equal(arrays[pre + 'p_' + n].astype(np.float32), params[n].numpy())
        for mode, train in MODES:
            with torch.no_grad():
                for n in names:
                    assert sd[n].shape == params[n].shape, n
                    sd[n].copy_(params[n])
            model.train(train)
            leaf = x.double().requires_grad_(True)
            y = model(leaf)
            named = dict(model.named_parameters())
            leaves = [n for n in names if R.is_leaf_name(n)]
            grads = torch.autograd.grad((y * up.double()).sum(), [leaf] + [named[n] for n in leaves])
            res = {'y': y.detach(), 'd_x': grads[0]}
            res.update({'d_' + n: g for n, g in zip(leaves, grads[1:])})
            if train:
                res.update({'new_' + n: sd[n].detach().clone() for n in names if not R.is_leaf_name(n)})
            for k, v in res.items():
                assert bool(v.ne(0).any()), (case, mode, k)
                arrays['%s%s_%s' % (pre, mode, k)] = v.numpy().astype(np.float32)
            # the plain-torch restatement agrees with what the reference just computed
            for dtype in (torch.float32, torch.float64):
                r = R.run_ref(x, params, net, up, train, dtype)
                worst = max(R.rel_err(r[k], res[k]) for k in res)
                print('%s %s, oracle %s: largest rel_err against the reference %.3e' % (case, mode, dtype, worst))
                assert worst <= 1e-6
        margins = {mode: R.tightest(R.leaky_margins(x, params, net, ups, train)) for mode, train in MODES}
        meta['seed'][case], meta['qualified'][case], meta['params'][case], meta['x'][case] = seed, len(good), names, list(xshape)
        meta['tightest_margin'][case] = {m: [t[0], t[1], t[2]] for m, t in margins.items()}
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'darknet_train.npz')
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg.npz'))      # the largest fixture


if __name__ == '__main__':
    main()
