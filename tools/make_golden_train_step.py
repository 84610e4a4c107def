"""Generate tests/golden/train_step.npz by EXECUTING THE REFERENCE's train-mode Yolact, MultiBoxLoss and torch.optim.SGD on the CPU (build
container only).

    python tools/make_golden_train_step.py          # needs the reference checkout; writes tests/golden/train_step.npz

The weights and inputs are those of tests/train_step_ref.build_case (the model of tests/test_gpu_stem_train.py's end-to-end case: seeded
ResNet-50 stages, 32 features, two 96 x 96 images), built from seeds by this repository's own containers and loaded into the reference's
Yolact through their common state-dict names.  The reference is imported with the stubs of oracle/make_golden._shim_reference.  Its
loop (train.py:215-216, 304-318) runs with a CONSTANT learning rate: zero_grad, forward in train mode, MultiBoxLoss, the sum of the
losses, backward, SGD(momentum cfg.momentum, weight_decay cfg.decay).step().  The candidates lr = 1e-3, 5e-4, 2.5e-4, 1e-4 are tried in
that order, and the first one for which the total loss of some iteration N <= 12 lies at least 10 % below that of iteration 0 is kept,
with the smallest such N.  Stored: lr, N, the totals of the iterations 0 .. N, the seeds.  Losses only: no weights.
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

LRS = (1e-3, 5e-4, 2.5e-4, 1e-4)
MAX_N = 12
DROP = 0.10
LOSS_SEED = 100          # torch.manual_seed(LOSS_SEED + iteration) before every iteration, in the test too


def main():
    import heads_train_ref as H
    import train_step_ref as T
    ours, images, targets, masks, num_crowds = T.build_case('cpu')
    state = {k: v.clone() for k, v in ours.state_dict().items()}
    import yolact_amd
    momentum, decay = yolact_amd.config.cfg.momentum, yolact_amd.config.cfg.decay
    from oracle.make_golden import _shim_reference
    _shim_reference()
    from data import cfg, set_cfg
    set_cfg('yolact_resnet50_config')
    o = H.golden_cfg_overrides()
    cfg.fpn = cfg.fpn.copy({'num_features': o.pop('num_features')})
    for k, v in o.items():
        setattr(cfg, k, v)
    assert (cfg.momentum, cfg.decay) == (momentum, decay) and not cfg.freeze_bn
    import yolact as ref_yolact
    from layers.modules import MultiBoxLoss
    torch.set_num_threads(H.helpers.ORACLE_THREADS)
    chosen = None
    for lr in LRS:
        net = ref_yolact.Yolact()
        net.load_state_dict(state)
        net.train()
        crit = MultiBoxLoss(cfg.num_classes, cfg.positive_iou_threshold, cfg.negative_iou_threshold, cfg.ohem_negpos_ratio)
        opt = torch.optim.SGD(net.parameters(), lr=lr, momentum=momentum, weight_decay=decay)
        totals = []
        for it in range(MAX_N + 1):
            torch.manual_seed(LOSS_SEED + it)
            opt.zero_grad()
            preds = net(images)
            losses = crit(net, preds, targets, masks, num_crowds)
            loss = sum(losses.values())
            loss.backward()
            assert bool(torch.isfinite(loss))
            opt.step()
            totals.append(float(loss.detach()))
            print('lr %g iteration %2d: total %.6f  %s' % (lr, it, totals[-1], {k: round(float(v), 4) for k, v in losses.items()}))
            if totals[-1] <= (1 - DROP) * totals[0]:
                chosen = (lr, it, totals)
                break
        if chosen:
            break
    assert chosen, 'no candidate learning rate makes the total loss fall by %d %% within %d iterations' % (100 * DROP, MAX_N)
    lr, n, totals = chosen
    meta = dict(case_seed=T.CASE_SEED, loss_seed=LOSS_SEED, momentum=momentum, decay=decay, torch=torch.__version__)
    dst = os.path.join(ROOT, 'tests', 'golden', 'train_step.npz')
    np.savez(dst, lr=np.float64(lr), N=np.int64(n), totals=np.array(totals, np.float64), total_0=np.float64(totals[0]),
             total_N=np.float64(totals[n]), meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
    print('lr %g, N %d: %.6f -> %.6f (%.1f %% lower); wrote %s' % (lr, n, totals[0], totals[n], 100 * (1 - totals[n] / totals[0]), dst))


if __name__ == '__main__':
    main()
