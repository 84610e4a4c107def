"""Generate tests/golden/fpn_train.npz by EXECUTING THE REFERENCE's own FPN class on the CPU (build container only).

    python tools/make_golden_fpn_train.py            # needs the reference checkout; writes tests/golden/fpn_train.npz
    python tools/make_golden_fpn_train.py --search N # which of the seeds 1 .. N qualify (needs no reference)

The reference is imported with the stubs of oracle/make_golden._shim_reference under yolact_resnet50_config with
fpn.num_features = 32; its FPN is built for in_channels = [64, 96, 128] and run at B = 2 on maps of 13 x 10, 7 x 5 and 4 x 3, which
gives P6 2 x 2 and P7 1 x 1: both interpolations (4 x 3 -> 7 x 5 -> 13 x 10) are no x2 in either axis, and both downsample layers see
an odd and an even extent.  The sixteen parameters are overwritten with known values.  Stored:

    c0 .. c2, p_<name>       the backbone maps (fp16) and the parameters (int16 numerators over 2048), on fp16-exact grids
                             (tests/fpn_train_ref.random_case, seed SEED)
    up_out0 .. 4             one fixed upstream gradient G_k per output, values in {-1, -1/2, 0, 1/2, 1} (three to a byte)
    q_out0 .. 4              the reference's five FPN outputs
    q_d_c0 .. 2, q_d_<name>  the gradients of sum_k <out_k, G_k> in the three maps and the sixteen parameters

SEED was chosen on the CPU so that every pred-layer pre-activation that receives gradient has at least 16 times that tensor's
fp32-versus-fp64 deviation as margin AND the fp32 restatement lies within 1e-6 (rel_err) of the fp64 one: 53 of the seeds 1 .. 64
qualify (QUALIFIED_OF_64; the margin alone fails the other 11, the 1e-6 distance holds for all 64: at most 6.3e-7), and SEED = 46 is the
one of them with the widest margin (2.3e-3 against a deviation of 4.7e-6).

The results are stored as integers of step max|v| * 2^-22 per array (tests/packed_fixture.pack).  Only data is stored.
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

SEED = 46
QUALIFIED_OF_64 = 53


def qualifies(R, seed):
    """(margin holds, fp32 within 1e-6 of fp64, tightest margin, worst distance) of a seed."""
    convouts, params, ups = R.random_case(seed, R.GOLDEN_IN, R.GOLDEN_NF, R.GOLDEN_SIZES, R.GOLDEN_B, R.GOLDEN_DOWN)
    m = R.relu_margins(convouts, params, R.GOLDEN_DOWN, ups)
    r64, r32 = (R.run_ref(convouts, params, R.GOLDEN_DOWN, ups, dt) for dt in (torch.float64, torch.float32))
    worst = max(R.rel_err(r32[k], r64[k]) for k in r64 if not k.startswith('_'))
    return all(lo >= 16 * dev for _, lo, dev in m), worst <= 1e-6, R.tightest(m), worst


def search(R, n):
    good, close = [], 0
    for seed in range(1, n + 1):
        margin, near, t, worst = qualifies(R, seed)
        close += near
        if margin and near:
            good.append(seed)
        print('seed %3d: margin %s (%s %.3e / %.3e), fp32 vs fp64 %.3e %s' % (seed, margin, t[0], t[1], t[2], worst, near))
    print('%d of the seeds 1 .. %d qualify (%d within 1e-6): %s' % (len(good), n, close, good))


def main():
    import fpn_train_ref as R
    if len(sys.argv) > 2 and sys.argv[1] == '--search':
        return search(R, int(sys.argv[2]))
    from oracle.make_golden import _shim_reference
    _shim_reference()
    from data import cfg, set_cfg
    set_cfg('yolact_resnet50_config')
    cfg.fpn = cfg.fpn.copy({'num_features': R.GOLDEN_NF})
    assert cfg.fpn.num_downsample == R.GOLDEN_DOWN and cfg.fpn.use_conv_downsample and cfg.fpn.relu_pred_layers and cfg.fpn.pad
    assert not cfg.fpn.relu_downsample_layers and cfg.fpn.interpolation_mode == 'bilinear'
    import yolact as ref_yolact
    fpn = ref_yolact.FPN(list(R.GOLDEN_IN))

    convouts, params, ups = R.random_case(SEED, R.GOLDEN_IN, R.GOLDEN_NF, R.GOLDEN_SIZES, R.GOLDEN_B, R.GOLDEN_DOWN)
    m = R.relu_margins(convouts, params, R.GOLDEN_DOWN, ups)
    print('tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % R.tightest(m))
    R.assert_margins(m)

    names = R.param_names(len(R.GOLDEN_IN), R.GOLDEN_DOWN)
    sd = fpn.state_dict()
    assert sorted('fpn.' + k for k in sd) == sorted(names), (list(sd), names)
    with torch.no_grad():
        for n in names:
            assert sd[n[4:]].shape == params[n].shape, n
            sd[n[4:]].copy_(params[n])
    leaves = [t.clone().requires_grad_(True) for t in convouts]
    torch.set_num_threads(R.helpers.ORACLE_THREADS)     # the thread count the oracle runs with on every host
    outs = fpn(leaves)
    assert [tuple(o.shape[2:]) for o in outs] == R.out_sizes(R.GOLDEN_SIZES, R.GOLDEN_DOWN) == [(13, 10), (7, 5), (4, 3), (2, 2), (1, 1)]
    named = {'fpn.' + k: v for k, v in fpn.named_parameters()}
    total = sum((o * u).sum() for o, u in zip(outs, ups))
    grads = torch.autograd.grad(total, leaves + [named[n] for n in names])

    arrays, steps, shapes = {}, {}, {}
    for i, t in enumerate(convouts):
        arrays['c%d' % i] = t.numpy().astype(np.float16)
    for n in names:
        arrays['p_' + n] = R.planes_of(torch.round(params[n] * R.PARAM_GRID).numpy(), 2)
    for i, u in enumerate(ups):
        arrays['up_out%d' % i] = R.pack5(u.numpy())
    results = {'out%d' % i: o.detach() for i, o in enumerate(outs)}
    results.update({'d_c%d' % i: g for i, g in enumerate(grads[:len(leaves)])})
    results.update({'d_' + n: g for n, g in zip(names, grads[len(leaves):])})
    for k, v in results.items():
        arrays['q_' + k], steps[k] = R.pack(v.numpy())
        shapes[k] = list(v.shape)

    # the plain-torch restatement agrees with what the reference just computed
    for dtype in (torch.float32, torch.float64):
        r = R.run_ref(convouts, params, R.GOLDEN_DOWN, ups, dtype)
        worst = max(R.rel_err(r[k], results[k]) for k in results)
        print('oracle %s: largest rel_err against the reference %.3e' % (dtype, worst))
        assert worst <= 1e-6

    meta = dict(seed=SEED, sizes=[list(s) for s in R.GOLDEN_SIZES], in_channels=list(R.GOLDEN_IN), B=R.GOLDEN_B, num_features=R.GOLDEN_NF,
                num_downsample=R.GOLDEN_DOWN, params=names, param_shapes={n: list(params[n].shape) for n in names}, steps=steps,
                shapes=shapes, qbits=R.QBITS, torch=torch.__version__)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'fpn_train.npz')
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg.npz'))      # the largest fixture


if __name__ == '__main__':
    main()
