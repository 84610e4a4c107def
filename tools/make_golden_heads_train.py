"""Generate tests/golden/heads_train.npz by EXECUTING THE REFERENCE's Yolact in train mode on the CPU (build container only).

    python tools/make_golden_heads_train.py          # needs the reference checkout; writes tests/golden/heads_train.npz

The reference is imported with the stubs of oracle/make_golden._shim_reference under yolact_resnet50_config with
fpn.num_features = 32, a 32-channel mask_proto_net and extra_head_net, num_classes = 6 and max_size = 96
(tests/heads_train_ref.golden_cfg_overrides).  A forward hook on its FPN returns five chosen leaves (12, 6, 3, 2, 1 squared, B = 2)
in place of the FPN's own output, so that the heads, the protonet and semantic_seg_conv see known inputs; the twenty head-side
parameters are overwritten with known values.  Stored:

    out0 .. out4, p_<name>   the leaves (fp16) and the parameters (int16 numerators over 2048), on fp16-exact grids (tests/heads_train_ref.random_case, seed SEED: chosen
                             on the CPU so that every ReLU decision that receives gradient has 16 times the fp32 deviation as margin
                             and the fp32 results lie within 1e-6 of the fp64 oracle: 17 of the seeds 1 .. 199 give the margin, the
                             sum over 1152 positions in d proto_net.8.weight puts 5 of those above 1e-6)
    up_<output>              one fixed upstream gradient G_k per output, values in {-1, -1/2, 0, 1/2, 1} (three to a byte)
    q_<output>               the reference's train-mode pred_outs: loc, conf, mask, proto, segm; priors as fp32
    q_d_out0 .. 4, q_d_<name>   the gradients of sum_k <pred_k, G_k> in the five leaves and the twenty parameters

The results are stored as integers of step max|v| * 2^-22 per array (tests/packed_fixture.pack: at most 1.2e-7 of the array's maximum
from the fp32 value), which keeps the file below the largest fixture.  Only data is stored.
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

SEED = 145


def main():
    from oracle.make_golden import _shim_reference
    _shim_reference()
    from data import cfg, set_cfg
    import heads_train_ref as H
    set_cfg('yolact_resnet50_config')
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    for k, v in o.items():
        setattr(cfg, k, v)
    import yolact as ref_yolact
    net = ref_yolact.Yolact()
    net.train()
    spec = H.spec_of(cfg)
    sizes = [(s, s) for s in H.GOLDEN_PYRAMID]
    outs, params, ups = H.random_case(SEED, spec, H.GOLDEN_NF, sizes, H.GOLDEN_B)
    m = H.relu_margins(outs, params, spec, ups)
    print('tightest ReLU margin: %s %.3e, fp32 deviation %.3e' % H.tightest(m))
    H.assert_margins(m)

    names = H.param_names(spec)
    sd = net.state_dict()
    head_keys = [k for k in sd if k.startswith(('proto_net.', 'prediction_layers.', 'semantic_seg_conv.'))]
    assert sorted(head_keys) == sorted(names), (head_keys, names)
    assert sum(sd[k].numel() for k in names) == 83875
    with torch.no_grad():
        for n in names:
            assert sd[n].shape == params[n].shape, n
            sd[n].copy_(params[n])
    leaves = [t.clone().requires_grad_(True) for t in outs]
    net.fpn.register_forward_hook(lambda module, inp, out: list(leaves))
    torch.manual_seed(0)
    torch.set_num_threads(H.helpers.ORACLE_THREADS)     # the thread count the oracle runs with on every host
    pred = net(torch.zeros(H.GOLDEN_B, 3, H.GOLDEN_MAX_SIZE, H.GOLDEN_MAX_SIZE))
    assert sorted(pred) == ['conf', 'loc', 'mask', 'priors', 'proto', 'segm'], sorted(pred)
    print({k: tuple(v.shape) for k, v in pred.items()})
    named = dict(net.named_parameters())
    total = sum((pred[k] * ups[k]).sum() for k in H.OUT_NAMES)
    grads = torch.autograd.grad(total, leaves + [named[n] for n in names])

    arrays, steps, shapes = {}, {}, {}
    f16 = lambda t: t.numpy().astype(np.float16)
    for i, t in enumerate(outs):
        arrays['out%d' % i] = f16(t)
    for n in names:
        arrays['p_' + n] = H.planes_of(torch.round(params[n] * H.PARAM_GRID).numpy(), 2)
    for k in H.OUT_NAMES:
        arrays['up_' + k] = H.pack5(ups[k].numpy())
    results = {k: pred[k].detach() for k in H.OUT_NAMES}
    results.update({'d_out%d' % i: g for i, g in enumerate(grads[:len(leaves)])})
    results.update({'d_' + n: g for n, g in zip(names, grads[len(leaves):])})
    for k, v in results.items():
        arrays['q_' + k], steps[k] = H.pack(v.numpy())
        shapes[k] = list(v.shape)
    arrays['priors'] = pred['priors'].detach().numpy().astype(np.float32)

    # the plain-torch restatement agrees with what the reference just computed
    for dtype in (torch.float32, torch.float64):
        r = H.run_ref(outs, params, spec, ups, dtype)
        worst = max(H.rel_err(r[k], results[k]) for k in results)
        print('oracle %s: largest rel_err against the reference %.3e' % (dtype, worst))
        assert worst <= 1e-6
        assert torch.equal(r['priors'], pred['priors'])

    meta = dict(seed=SEED, pyramid=list(H.GOLDEN_PYRAMID), B=H.GOLDEN_B, num_features=H.GOLDEN_NF, num_classes=H.GOLDEN_CLASSES,
                max_size=H.GOLDEN_MAX_SIZE, params=names, param_shapes={n: list(params[n].shape) for n in names}, steps=steps, shapes=shapes, qbits=H.QBITS, torch=torch.__version__)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'heads_train.npz')
    np.savez_compressed(out, **arrays)
    print('wrote', out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) <= os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'jpeg.npz'))      # the largest fixture


if __name__ == '__main__':
    main()
